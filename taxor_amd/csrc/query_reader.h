// query_reader.h -- one query file -> numbered chunks of records (fastx::Batch) from a recycling buffer pool.  produce_batches() sniffs
// the file and picks one of four readers: byte ranges of a plain file, BAM, parallel gzip (a cutter plus a parser pool), or the
// sequential reader.  Used by `taxor search` (search_cmd.h) and `taxor reads` (tools_cmd.h).  Included by search_main.cpp inside its
// anonymous namespace, after cli_util.h.

using fastx::Batch;

// a chunk's page-locked buffers back to pageable memory: before they are freed (a registration over freed memory would be a DMA
// source the allocator hands out again) -- the pool's trim and the teardown between two index files both come through here
inline void unpin_buffers(Batch &b)
{
    if (b.pinned) { taxor_gpu_host_unregister(b.pinned); b.pinned = nullptr; }
    if (b.raw_pinned) { taxor_gpu_host_unregister(b.raw_pinned); b.raw_pinned = nullptr; }
}

// a recycled chunk whose `raw` buffer last held file bytes or a BAM batch, refilled by a parser that never touches `raw`: the buffer
// (up to 64 MB and more, page-locked) goes back instead of travelling with the chunk unused
inline void drop_raw(Batch &b)
{
    if (b.raw_pinned) { taxor_gpu_host_unregister(b.raw_pinned); b.raw_pinned = nullptr; }
    if (b.raw.capacity()) b.raw.release();
}

// Finished batches go back to the producers: their buffers stay mapped and warm, and at most `cap` batches exist at
// a time (get() blocks), which bounds the host memory the pipeline touches -- faulting in and releasing fresh pages
// costs more than parsing into them.
// The bound is in BYTES as well as in buffers: a chunk's sequence buffer is ~128 MB, page-locked, and recycled rather than
// released, so a count sized for the deepest queues (~150 buffers for one device, ~600 for eight) would let a run whose
// parsers outrun the GPUs or the writer pin tens of gigabytes.  Beyond `floor` buffers -- what the stages need to hold one
// each, so that the pipeline can never starve itself -- a new buffer is made only while the bytes of the existing ones stay
// within `byte_budget`, and a buffer that comes back while the pool is over budget is released (unregistered and freed)
// instead of kept.
struct BatchPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::unique_ptr<Batch>> free_;
    size_t cap = 8, made = 0, floor = 8;
    uint64_t byte_budget = ~0ull, bytes = 0;   // bytes: sequence-buffer capacity of every live batch, as of its last return
    uint64_t peak_bytes = 0, trimmed = 0;
    std::unique_ptr<Batch> get()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !free_.empty() || (made < cap && (made < floor || bytes < byte_budget)); });
        if (free_.empty()) { ++made; return std::make_unique<Batch>(); }
        auto b = std::move(free_.back());
        free_.pop_back();
        return b;
    }
    void put(std::unique_ptr<Batch> b)
    {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t now_bytes = b->bases.capacity() + b->raw.capacity();
        bytes += now_bytes - b->pool_bytes;
        b->pool_bytes = now_bytes;
        peak_bytes = std::max(peak_bytes, bytes);
        if (bytes > byte_budget && made > floor) {      // over budget: this buffer goes back to the system
            bytes -= now_bytes;
            --made;
            ++trimmed;
            lk.unlock();
            unpin_buffers(*b);
            b.reset();
            cv.notify_one();
            return;
        }
        free_.push_back(std::move(b));
        cv.notify_one();
    }
};

// what the readers take from the command line (`taxor search`'s Config extends it)
struct ReaderOptions {
    unsigned threads = 0;       // 0 = not given: as many host threads as feed one GPU (see parse_search_args); the reference's default is ONE worker
    uint64_t batch_reads = 0, batch_bases = 1ull << 30;   // 0 reads: 65536 per batch (sequential reader) or ~128 MB of
                                                           // file per batch (plain file, parsed in parallel)
    bool device_parse = false;  // --device-parse: byte ranges of plain files go to the device as read; it finds the records
};

// Where a file's readers get their buffers and leave their chunks: the gate (a file may not run too far ahead of the one being
// written), the pool, the consumer, and the count the end-of-file marker carries.  push() is called from several threads.
struct ChunkSink {
    BatchPool &pool;
    const std::function<void(std::unique_ptr<Batch>)> &out;
    const std::function<void()> &gate;
    uint32_t file;
    std::atomic<uint64_t> n_pushed{0};
    std::unique_ptr<Batch> get() { if (gate) gate(); return pool.get(); }
    void push(std::unique_ptr<Batch> b)
    {
        b->file = file;
        b->end_of_file = false;
        ++n_pushed;
        out(std::move(b));
    }
    void finish()      // tells the consumer how many chunks this file had
    {
        auto m = std::make_unique<Batch>();
        m->file = file;
        m->seq = n_pushed.load();
        m->end_of_file = true;
        m->offsets.assign(1, 0);
        out(std::move(m));
    }
};

// One parser thread's reader and what it remembers from chunk to chunk.
struct ChunkParser {
    fastx::FastxReader rd;
    std::string id;
    size_t prev_records = 0, prev_id_bytes = 0;

    // a recycled chunk, made ready for up to `need` bases
    void prepare(Batch &bt, size_t need)
    {
        if (need > bt.bases.capacity()) {  // grow before parsing, and only with the old block unpinned
            if (bt.pinned) { taxor_gpu_host_unregister(bt.pinned); bt.pinned = nullptr; }
            bt.bases.clear();
            bt.bases.reserve((need + need / 16 + (2u << 20)) & ~size_t((2u << 20) - 1));
            // a fresh 128-MB buffer is 32768 page faults when it is first written -- for a query file smaller than the
            // pool, every buffer is fresh; as huge pages it is 64 (where the system allows them on request)
            const uintptr_t a = ((uintptr_t)&bt.bases[0] + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
            const uintptr_t e = ((uintptr_t)&bt.bases[0] + bt.bases.capacity()) & ~(uintptr_t)((2u << 20) - 1);
            if (e > a) (void)madvise((void *)a, e - a, MADV_HUGEPAGE);
        }
        bt.ids.clear();
        bt.bases.clear();
        bt.offsets.assign(1, 0);
        // a fresh chunk buffer: size the per-record arrays once, from what the previous chunk of this thread
        // held (growing a vector of 10^5 entries by doubling is a dozen reallocations, each an mmap/munmap
        // and a TLB shootdown across every thread of the process)
        const size_t guess = prev_records + prev_records / 8 + 1024;
        if (bt.offsets.capacity() < guess) bt.offsets.reserve(guess + 1);
        if (bt.ids.off.capacity() < guess || bt.ids.data.capacity() < prev_id_bytes) bt.ids.reserve(guess, prev_id_bytes + prev_id_bytes / 8 + 4096);
    }
    // every record `rd` (opened by the caller) still holds, appended to the chunk
    void parse(Batch &bt)
    {
        while (rd.next(id, bt.bases)) {
            bt.ids.push_back(id);
            bt.offsets.push_back(bt.bases.size());
        }
        prev_records = bt.ids.size();
        prev_id_bytes = bt.ids.data.size();
    }
};

// --device-parse: the range [b, e) as it is in the file -- the GPU worker hands it to the device's scanner
void fill_raw_range(Batch &bt, const fastx::RangedFastx &rf, uint64_t b, uint64_t e)
{
    const size_t len = (size_t)(e - b);
    bt.ids.clear();
    bt.bases.clear();
    bt.offsets.assign(1, 0);
    bt.may_pin = false;
    // the bytes go to the device from here: the buffer is page-locked once, when it is made or grown, and
    // recycled with the chunk like the parsed chunks' sequence buffers (the copy is then DMA, not a staging
    // copy on the thread that feeds the GPU)
    if (len > bt.raw.capacity()) {
        if (bt.raw_pinned) { taxor_gpu_host_unregister(bt.raw_pinned); bt.raw_pinned = nullptr; }
        bt.raw.clear();
        bt.raw.reserve((len + len / 16 + (2u << 20)) & ~size_t((2u << 20) - 1));
    }
    bt.raw.clear();
    bt.raw.resize(len);
    if (!bt.raw_pinned && taxor_gpu_host_register(bt.raw.data(), bt.raw.capacity()) == TAXOR_OK) bt.raw_pinned = bt.raw.data();
    for (size_t got = 0; got < len;) {
        const ssize_t r = pread(rf.fd, bt.raw.data() + got, len - got, (off_t)(b + got));
        if (r <= 0) throw std::runtime_error("query file: read error");
        got += (size_t)r;
    }
    bt.raw_kind = rf.kind;
}

// A plain file: `nt` threads, each taking the next byte range of about cfg.batch_reads records and parsing it (or, under
// --device-parse, reading it as it is).
void read_byte_ranges(fastx::RangedFastx &rf, const ReaderOptions &cfg, unsigned nt, ChunkSink &sink)
{
    if (cfg.batch_reads) rf.plan(cfg.batch_reads, std::min<uint64_t>(cfg.batch_bases, 1ull << 30));
    else rf.range_bytes = rf.kind == '@' ? (128u << 20) : (64u << 20);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&] {
            ChunkParser ps;
            uint64_t b, e, seq;
            for (;;) {
                auto bt = sink.get();                   // buffer first: ranges are then taken in the order they can be filled
                try {
                    if (!rf.next_range(b, e, seq)) { sink.pool.put(std::move(bt)); break; }
                    bt->seq = seq;
                    bt->may_pin = true;
                    ++bt->fills;
                    if (cfg.device_parse) fill_raw_range(*bt, rf, b, e);
                    else {
                        drop_raw(*bt);
                        ps.prepare(*bt, fastx::bases_bound(e - b, rf.kind));
                        ps.rd.open_range(rf.fd, b, e, rf.kind == '@');
                        ps.parse(*bt);
                    }
                } catch (const std::exception &ex) { die(ex.what()); }
                sink.push(std::move(bt));
            }
        });
    for (auto &t : th) t.join();
}

// BAM (bam.h): the blocks are inflated on this file's threads (one zlib stream without allow_ranges), this thread walks the
// records and copies their 4-bit SEQ fields back to back into the chunk's raw buffer, which goes to the device as it is.
// With --batch-reads a chunk is exactly that many records, like the sequential FASTX reader's below.  Without, chunks are
// cut by size, in the class of the range readers' (128 MB of FASTQ text hold 64 MB of SEQ bytes): at 2^27 bases, so that the
// GPU starts on the first chunk while the walker fills the second -- a cut by records alone made ONE chunk of a file of
// long reads.  Either rule depends on the file alone: the paged route, which reads the file once per pass, gets the same
// chunks every time.  The buffer is page-locked by the pinner stage behind this thread (search_cmd.h), never here.
// Returns the time spent waiting for the consumers.
double read_bam(const std::string &query, const ReaderOptions &cfg, bool allow_ranges, unsigned bam_threads, ChunkSink &sink, double t_begin)
{
    const uint64_t batch_reads = cfg.batch_reads ? cfg.batch_reads : (1u << 20);
    const uint64_t batch_bases = cfg.batch_reads ? cfg.batch_bases : std::min<uint64_t>(cfg.batch_bases, 1ull << 27);
    uint64_t seq = 0;
    double blocked = 0;
    try {
        bam::Reader rd;
        rd.open(query, bam_threads, !allow_ranges);
        Batch *cur = nullptr;
        // a buffer that is page-locked where it stands: the registration is given up before the buffer moves
        rd.grow = [&](size_t) { if (cur && cur->raw_pinned) { taxor_gpu_host_unregister(cur->raw_pinned); cur->raw_pinned = nullptr; } };
        for (bool more = true; more;) {
            auto b = sink.get();
            cur = b.get();
            b->seq = seq++;
            b->may_pin = false;
            b->ids.clear();
            b->bases.clear();
            b->raw.clear();
            b->offsets.assign(1, 0);
            b->nib_off.clear();
            b->nib_len.clear();
            b->nib_rev.clear();
            if (!cfg.batch_reads && b->raw.capacity() < (batch_bases / 2 + (4u << 20))) {      // sized once: a size-cut chunk never grows past this
                rd.grow(0);
                b->raw.reserve(batch_bases / 2 + (4u << 20));
            }
            while (b->ids.size() < batch_reads && b->offsets.back() < batch_bases && (more = rd.next(b->ids, b->raw, b->nib_off, b->nib_len, b->nib_rev)))
                b->offsets.push_back(b->offsets.back() + b->nib_len.back());
            cur = nullptr;
            if (b->ids.empty()) { sink.pool.put(std::move(b)); break; }
            b->raw_kind = 'B';
            const double t1 = now();
            sink.push(std::move(b));
            blocked += now() - t1;
        }
        if (tune_env("TAXOR_CLI_TRACE"))
            fprintf(stderr, "[trace] BAM %s: %llu records, %llu skipped as secondary or supplementary (flag & 0x900), blocks inflated %s, %llu chunks, walker %.3f s\n",
                    query.c_str(), (unsigned long long)rd.ordinal, (unsigned long long)rd.n_skipped, rd.use_members ? "in parallel" : "as one zlib stream",
                    (unsigned long long)sink.n_pushed.load(), now() - t_begin - blocked);
    } catch (const std::exception &ex) { die(ex.what()); }
    return blocked;
}

// Front to back on this thread, batches cut at exactly cfg.batch_reads records.  Returns the time spent waiting for the consumers.
double read_sequential(fastx::FastxReader &rd, const ReaderOptions &cfg, ChunkSink &sink)
{
    std::string id;
    bool more = true;
    uint64_t seq = 0;
    double blocked = 0;
    const uint64_t batch_reads = cfg.batch_reads ? cfg.batch_reads : 65536;
    try {
        while (more) {
            auto b = sink.get();
            // a batch recycled from the ranged reader of an earlier plain file may still be page-locked; this reader
            // appends without a size bound, so the string can reallocate: give the registration up first (a stale
            // registration over freed memory would be a DMA source) and do not pin batches of this path again
            if (b->pinned) { taxor_gpu_host_unregister(b->pinned); b->pinned = nullptr; }
            drop_raw(*b);
            b->may_pin = false;
            b->seq = seq++;
            b->ids.clear();
            b->bases.clear();
            b->offsets.assign(1, 0);
            while (b->ids.size() < batch_reads && b->bases.size() < cfg.batch_bases && (more = rd.next(id, b->bases))) {
                b->ids.push_back(id);
                b->offsets.push_back(b->bases.size());
            }
            if (b->ids.empty()) { sink.pool.put(std::move(b)); break; }
            const double t1 = now();
            sink.push(std::move(b));
            blocked += now() - t1;
        }
    } catch (const std::exception &ex) { die(ex.what()); }
    return blocked;
}

// ---- parallel gzip.  The inflated stream arrives in chunks of ~16 MB that change hands without a copy (ParallelGz::take); a
// multi-member file -- bgzip's 64-KB members, concatenated runs -- goes the same way, its members being the chunks.  The cutter
// (the file's reader thread) only CUTS: it collects chunks up to ~64 MB, finds the last record start in the last one (the range
// reader's test: an '@' line whose second successor starts with '+', or a '>' line), and hands everything before it -- whole
// records -- to a parser thread; what follows the cut is carried into the next segment.  The parsers work like those of a plain
// file's byte ranges, the buffers are their input directly.  A file whose first records are not of the kind the cut can recognise
// (FASTQ that wraps its lines) is parsed front to back on the reader thread instead.
struct GzSource {
    fastx::GzMembers members;
    fastx::ParallelGz pgz;
    bool single = false, multi = false;     // one member inflated speculatively from the middle (pgz.h) / members as chunks
    bool take(std::vector<char> &v) { return single ? pgz.take(v) : members.take(v); }
};

struct GzJob { std::deque<std::vector<char>> parts; uint64_t seq = 0; size_t bytes = 0; };

// the cutter's hand-over to its parsers: at most np + 2 jobs wait
struct GzJobs {
    std::mutex mu;
    std::condition_variable cv_put, cv_get;
    std::deque<GzJob> jobs;
    bool done = false;
    unsigned np = 2;
    uint64_t next_seq = 0;      // the cutter's alone
    void submit(GzJob &&j)
    {
        if (j.bytes == 0) return;
        j.seq = next_seq++;
        std::unique_lock<std::mutex> lk(mu);
        cv_put.wait(lk, [&] { return jobs.size() < np + 2; });
        jobs.push_back(std::move(j));
        cv_get.notify_one();
    }
    bool next(GzJob &job)       // false once closed and drained
    {
        std::unique_lock<std::mutex> lk(mu);
        cv_get.wait(lk, [&] { return !jobs.empty() || done; });
        if (jobs.empty()) return false;
        job = std::move(jobs.front());
        jobs.pop_front();
        cv_put.notify_one();
        return true;
    }
    void close()
    {
        { std::lock_guard<std::mutex> lk(mu); done = true; }
        cv_get.notify_all();
    }
};

// whether the cutter can recognise the record starts of text that begins at p with a record of `kind`
bool gz_cuttable(char kind, const char *p, const char *e)
{
    bool cuttable = kind == '>' || kind == '@';
    if (kind == '@')
        for (int rec = 0; rec < 16 && p < e && cuttable; ++rec) {
            const char *l3 = fastx::next_line(fastx::next_line(p, e), e);
            if (l3 >= e) break;
            if (*l3 != '+') cuttable = false;
            const char *nx = fastx::next_line(fastx::next_line(l3, e), e);
            if (nx < e && *nx != '@' && *nx != '\n' && *nx != '\r') cuttable = false;
            p = nx;
        }
    return cuttable;
}

void gz_parser(GzJobs &jobs, GzSource &gz, char kind, ChunkSink &sink)
{
    ChunkParser ps;
    if (gz.single) ps.rd.mem_recycle = [&gz](std::vector<char> &&v) { gz.pgz.recycle(std::move(v)); };
    for (GzJob job; jobs.next(job);) {
        auto bt = sink.get();
        try {
            bt->seq = job.seq;
            bt->may_pin = true;
            ++bt->fills;
            drop_raw(*bt);
            ps.prepare(*bt, fastx::bases_bound(job.bytes, kind));
            ps.rd.open_mem(std::move(job.parts), kind == '@');
            ps.parse(*bt);
        } catch (const std::exception &ex) { die(ex.what()); }
        sink.push(std::move(bt));
    }
}

// the cutter: `first` is the stream's first chunk, beginning at a record start; `target` = bytes of text per parser job
void gz_cut(GzJobs &jobs, GzSource &gz, std::vector<char> &&first, char kind, size_t target)
{
    GzJob cur;
    auto add = [&](std::vector<char> &&v) { cur.bytes += v.size(); cur.parts.push_back(std::move(v)); };
    add(std::move(first));
    for (;;) {
        if (cur.bytes >= target) {
            // the last record start in the last part, looked for in its final megabyte (a record is tens of kilobytes)
            std::vector<char> &last = cur.parts.back();
            const char *b = last.data(), *e = b + last.size();
            const char *w = last.size() > (1u << 20) ? e - (1u << 20) : b;
            // (a part starts at a line start only if it is the job's first: jobs begin at record starts; a bgzip member begins anywhere)
            const char *p = w == b && cur.parts.size() == 1 ? b : fastx::next_line(w, e);
            const char *cut = nullptr;
            for (const char *r = fastx::resync(p, e, kind); r < e; r = fastx::resync(fastx::next_line(r, e), e, kind)) cut = r;
            if (cut && (cut > b || cur.parts.size() > 1)) {
                std::vector<char> carry(cut, e);
                cur.bytes -= (size_t)(e - cut);
                last.resize((size_t)(cut - b));
                GzJob next;
                next.bytes = carry.size();
                next.parts.push_back(std::move(carry));
                jobs.submit(std::move(cur));
                cur = std::move(next);
            }
        }
        std::vector<char> ck;
        if (!gz.take(ck)) break;
        if (!ck.empty()) add(std::move(ck));
    }
    jobs.submit(std::move(cur));
}

// gzip, bzip2, pipes, --sequential: the parallel gzip route where the file and the options allow it, else (or from its first chunk
// on, where the text cannot be cut) the sequential reader.  Returns the time the sequential reader spent waiting for the consumers.
double read_compressed(const std::string &query, const ReaderOptions &cfg, bool allow_ranges, unsigned parse_threads, ChunkSink &sink)
{
    fastx::FastxReader rd;
    GzSource gz;
    // (inflating threads: up to 32 of --threads -- or what the container's CPU quota allows: beyond it the cgroup only stops them all)
    static const unsigned gz_cap = [] { const double q = cpu_quota(); return q >= 1.0 ? std::min(32u, std::max(2u, (unsigned)q)) : 32u; }();
    const unsigned gz_threads = parse_threads ? parse_threads : std::max(1u, std::min(cfg.threads, gz_cap));
    try {
        gz.multi = allow_ranges && gz.members.open(query, gz_threads);
        // one member (what `gzip reads.fastq` writes): inflated speculatively from the middle on all of this file's threads (pgz.h);
        // --sequential and small files keep the one zlib stream
        if (!gz.multi && allow_ranges && gz_threads > 1) gz.single = gz.pgz.open(query, gz_threads);
    } catch (const std::exception &ex) { die(ex.what()); }
    if (!gz.single && !gz.multi) {
        if (!rd.open(query)) die("cannot open query file " + query);
        return read_sequential(rd, cfg, sink);
    }
    std::vector<char> first;
    bool have = false;
    try {
        while ((have = gz.take(first)) && first.empty()) {}         // (empty members are legal)
    } catch (const std::exception &ex) { die(ex.what()); }
    size_t i0 = 0;
    while (i0 < first.size() && (first[i0] == '\n' || first[i0] == '\r')) ++i0;
    const char kind = have && i0 < first.size() ? first[i0] : 0;
    const bool cuttable = gz_cuttable(kind, first.data() + i0, first.data() + std::min<size_t>(first.size(), i0 + (1u << 16)));
    if (have && kind && !cuttable && kind != '@' && kind != '>') die("query file is neither FASTA nor FASTQ");
    if (!have || !cuttable) {
        if (gz.single) rd.pgz = &gz.pgz;                       // front to back: the chunk already taken first, then the stream
        else rd.members = &gz.members;
        rd.buf.swap(first);
        rd.pos = 0;
        rd.len = rd.buf.size();
        if (rd.buf.size() < (8u << 20)) rd.buf.resize(8u << 20);
        if (gz.single) gz.pgz.switch_to_read();
        return read_sequential(rd, cfg, sink);
    }
    GzJobs jobs;
    static const unsigned np_env = [] { const char *e = tune_env("TAXOR_CLI_GZ_PARSERS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 64 ? (unsigned)v : 0u; }();
    jobs.np = np_env ? np_env : std::max(2u, gz_threads / 4);
    std::vector<std::thread> parsers;
    for (unsigned t = 0; t < jobs.np; ++t) parsers.emplace_back([&] { gz_parser(jobs, gz, kind, sink); });
    try {
        if (i0) first.erase(first.begin(), first.begin() + (long)i0);
        gz_cut(jobs, gz, std::move(first), kind, (size_t)std::min<uint64_t>(cfg.batch_bases, kind == '@' ? (64u << 20) : (32u << 20)));
    } catch (const std::exception &ex) { die(ex.what()); }
    jobs.close();
    for (auto &t : parsers) t.join();
    return 0;
}

// Numbered batches of records from one query file -> push_() (called from several threads, batches may arrive out
// of order; `seq` gives the input order).  Returns the wall time spent producing.
double produce_batches(const std::string &query, const ReaderOptions &cfg, bool allow_ranges, BatchPool &pool,
                       const std::function<void(std::unique_ptr<Batch>)> &push_, uint32_t file = 0, unsigned parse_threads = 0,
                       const std::function<void()> &gate = nullptr)
{
    ChunkSink sink{pool, push_, gate, file};
    const double t_begin = now();
    double blocked = 0;   // time a reader that fills one chunk at a time spent waiting for the consumers
    fastx::RangedFastx rf;
    bool ranged = false, is_bam = false;
    try {
        is_bam = bam::sniff(query) == bam::BAM;      // by content, never by name; CRAM and SAM text are refused by name
        ranged = !is_bam && allow_ranges && rf.open(query);
    } catch (const std::exception &e) { die(e.what()); }
    if (ranged) read_byte_ranges(rf, cfg, parse_threads ? parse_threads : std::max(1u, std::min(cfg.threads, 16u)), sink);
    else {
        if (cfg.device_parse) {
            static std::atomic<bool> said{false};
            if (!said.exchange(true)) {
                if (is_bam) fprintf(stderr, "--device-parse: %s is BAM: the switch is ignored (its records are walked on the host and its sequences unpacked on the device in any case)\n", query.c_str());
                else fprintf(stderr, "--device-parse: %s is compressed or read sequentially: it is parsed on the host\n", query.c_str());
            }
        }
        if (is_bam) blocked = read_bam(query, cfg, allow_ranges, parse_threads ? parse_threads : std::max(1u, std::min(cfg.threads, 32u)), sink, t_begin);
        else blocked = read_compressed(query, cfg, allow_ranges, parse_threads, sink);
    }
    sink.finish();
    return now() - t_begin - blocked;
}
