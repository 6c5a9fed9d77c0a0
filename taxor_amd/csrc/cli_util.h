// cli_util.h -- what every subcommand of the `taxor` executable shares: the bounded queue between pipeline stages, die / now / trace,
// CPU-time and cgroup marks, and a few string and file helpers.  Included by search_main.cpp inside its anonymous namespace, first.

template <typename T> class BoundedQueue {
public:
    explicit BoundedQueue(size_t cap) : cap_(cap) {}
    void push(T v)
    {
        std::unique_lock<std::mutex> lk(m_);
        not_full_.wait(lk, [&] { return q_.size() < cap_; });
        q_.push_back(std::move(v));
        not_empty_.notify_one();
    }
    bool pop(T &out) // false once closed and drained
    {
        std::unique_lock<std::mutex> lk(m_);
        not_empty_.wait(lk, [&] { return !q_.empty() || closed_; });
        return take(out);
    }
    bool pop_for(T &out, double seconds) // like pop, but gives up (false) after `seconds`
    {
        std::unique_lock<std::mutex> lk(m_);
        not_empty_.wait_for(lk, std::chrono::duration<double>(seconds), [&] { return !q_.empty() || closed_; });
        return take(out);
    }
    bool try_pop(T &out) // false if nothing is queued right now
    {
        std::lock_guard<std::mutex> lk(m_);
        return take(out);
    }
    bool done() // closed and drained
    {
        std::lock_guard<std::mutex> lk(m_);
        return closed_ && q_.empty();
    }
    void close()
    {
        std::lock_guard<std::mutex> lk(m_);
        closed_ = true;
        not_empty_.notify_all();
    }

private:
    bool take(T &out) // with m_ held
    {
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        not_full_.notify_one();
        return true;
    }
    std::mutex m_;
    std::condition_variable not_full_, not_empty_;
    std::deque<T> q_;
    size_t cap_;
    bool closed_ = false;
};

std::vector<std::string> str_split(const std::string &s, char delim)         // taxor_search.cpp:82-95
{
    std::vector<std::string> out;
    size_t a = 0;
    while (a <= s.size()) {
        const size_t b = s.find(delim, a);
        if (b == std::string::npos) { if (a < s.size()) out.push_back(s.substr(a)); break; }
        out.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return out;
}

bool file_exists(const std::string &p)
{
    struct stat sb;
    return stat(p.c_str(), &sb) == 0;
}

[[noreturn]] void die(const std::string &msg)
{
    fprintf(stderr, "[TAXOR SEARCH ERROR] %s\n", msg.c_str());             // :380-384
    exit(-1);
}

uint64_t fnv1a(const char *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
    return h;
}

double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// CPU time of the process so far and what the cgroup's CPU quota took away (cpu.max: a container is commonly given fewer CPUs than
// the machine shows -- the pool's GPU box 16 of 256 -- and every thread of the process stops for the rest of a 100-ms period once
// the quota of that period is used up)
struct CpuMark { double user = 0, sys = 0, throttled = 0; uint64_t periods = 0, throttled_periods = 0; };
CpuMark cpu_mark()
{
    CpuMark m;
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    m.user = ru.ru_utime.tv_sec + 1e-6 * ru.ru_utime.tv_usec;
    m.sys = ru.ru_stime.tv_sec + 1e-6 * ru.ru_stime.tv_usec;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.stat", "r")) {
        char key[64];
        unsigned long long v;
        while (fscanf(f, "%63s %llu", key, &v) == 2) {
            if (!strcmp(key, "nr_periods")) m.periods = v;
            else if (!strcmp(key, "nr_throttled")) m.throttled_periods = v;
            else if (!strcmp(key, "throttled_usec")) m.throttled = v * 1e-6;
        }
        fclose(f);
    }
    return m;
}
// CPUs the container's cgroup allows (cpu.max: quota / period); 0 if there is no quota
double cpu_quota()
{
    double q = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char a[64];
        unsigned long long period = 0;
        if (fscanf(f, "%63s %llu", a, &period) == 2 && strcmp(a, "max") != 0 && period) q = (double)strtoull(a, nullptr, 10) / (double)period;
        fclose(f);
    }
    return q;
}
// CPUs the process may use: the smaller of the affinity mask and the cgroup's quota (0 if unknown)
double cpu_allowance()
{
    const double q = cpu_quota();
    cpu_set_t set;
    CPU_ZERO(&set);
    const double aff = sched_getaffinity(0, sizeof set, &set) == 0 ? (double)CPU_COUNT(&set) : 0.0;
    return q > 0 && aff > 0 ? std::min(q, aff) : std::max(q, aff);
}

// TAXOR_CLI_TRACE=1: wall-clock marks of the pipeline stages on stderr
const double g_t0 = now();
void trace(const char *what)
{
    static const bool on = tune_env("TAXOR_CLI_TRACE") != nullptr;
    if (on) fprintf(stderr, "[trace] %8.3f s  %s\n", now() - g_t0, what);
}
