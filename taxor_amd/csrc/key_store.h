// key_store.h -- the host side of a `taxor build` whose keys do not fit in device memory ("Beyond device
// memory"): the store the keyer's waves are appended to, the cut of the genomes into waves, the offsets of a split bin's parts, and
// the two refusals that are decided from numbers alone.  No HIP in here: tests/sanitize/key_store_check.cpp runs it under ASan + UBSan.
#pragma once
#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace taxor {

// Part j of `parts` of a bin whose m sorted keys start at `first`: [first + m*j/parts, first + m*(j+1)/parts) -- the rule of
// taxor_build_layout (a split user bin is contiguous parts of its sorted keys), so a part is a range of the store and nothing moves.
inline void key_part_range(uint64_t first, uint64_t m, uint64_t parts, uint64_t j, uint64_t *part_first, uint64_t *part_count)
{
    const unsigned __int128 mm = m;
    const uint64_t lo = (uint64_t)(mm * j / parts), hi = (uint64_t)(mm * (j + 1) / parts);
    *part_first = first + lo;
    *part_count = hi - lo;
}

// Upper bound of the distinct keys a genome file of `file_bytes` can bring (compressed files hold more bases than bytes: x4;
// syncmers: one key per min(t, k-s+1-t+1) bases at the densest, minimisers: one per base)
inline uint64_t key_bound_of_file(uint64_t file_bytes, bool compressed, bool use_syncmer, int k, int s, int t)
{
    const uint64_t bases = compressed ? 4 * file_bytes : file_bytes;
    const int d = use_syncmer ? (t < k - s + 1 - t + 1 ? t : k - s + 1 - t + 1) : 1;
    return bases / (uint64_t)(d < 1 ? 1 : d) + 1;
}

// Genomes [wave_first[w], wave_first[w+1]) are keyed together: consecutive genomes (taxonomy order) while their key bounds fit
// `budget_keys`.  Returns the index of a genome whose own bound exceeds the budget (nothing is cut then), or -1.
inline int64_t cut_waves(const std::vector<uint64_t> &key_bound, uint64_t budget_keys, std::vector<uint64_t> &wave_first)
{
    wave_first.assign(1, 0);
    uint64_t in_wave = 0;
    for (uint64_t g = 0; g < key_bound.size(); ++g) {
        if (key_bound[g] > budget_keys) return (int64_t)g;
        if (in_wave + key_bound[g] > budget_keys) {
            wave_first.push_back(g);
            in_wave = 0;
        }
        in_wave += key_bound[g];
    }
    wave_first.push_back(key_bound.size());
    return -1;
}

// MemAvailable of /proc/meminfo in bytes (0: not known)
inline uint64_t host_memory_available(const char *meminfo_path = "/proc/meminfo")
{
    FILE *f = fopen(meminfo_path, "r");
    if (!f) return 0;
    char line[256];
    uint64_t kb = 0;
    while (fgets(line, sizeof line, f))
        if (strncmp(line, "MemAvailable:", 13) == 0) {
            kb = strtoull(line + 13, nullptr, 10);
            break;
        }
    fclose(f);
    return kb << 10;
}

// "" when a store of up to `bound_keys` keys fits the host's available memory, else the refusal's text with both figures
inline std::string host_store_refusal(uint64_t bound_keys, uint64_t available_bytes)
{
    const unsigned __int128 need = (unsigned __int128)bound_keys * 8;
    if (available_bytes && need <= available_bytes) return "";
    if (!available_bytes) return "";                       // no figure to hold against: the allocation itself decides
    return "the distinct keys of these genomes may need " + std::to_string((uint64_t)(need >> 20)) + " MiB of host memory, " +
           std::to_string(available_bytes >> 20) + " MiB are available; keys on disk are not supported";
}

// All distinct keys of a build, bin after bin: ONE array in address space, reserved for the bound at once and backed by the
// kernel page by page as the waves arrive (no vector that grows by copying itself, and no memory for the gap between the density
// bound and what the genomes really hold).
class KeyStore {
public:
    KeyStore() = default;
    KeyStore(const KeyStore &) = delete;
    KeyStore &operator=(const KeyStore &) = delete;
    ~KeyStore() { release(); }

    bool reserve(uint64_t cap_keys)
    {
        release();
        cap_ = cap_keys ? cap_keys : 1;
        void *p = mmap(nullptr, cap_ * 8, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { cap_ = 0; return false; }
        keys_ = static_cast<uint64_t *>(p);
        bin_off_.assign(1, 0);
        return true;
    }

    // the keys of the next n_bins bins: bin b's are src[off[b] - off[0], off[b+1] - off[0])
    bool append(const uint64_t *src, const uint64_t *off, uint64_t n_bins)
    {
        const uint64_t n = off[n_bins] - off[0];
        if (n > cap_ - size()) return false;
        if (n) memcpy(keys_ + size(), src, n * 8);
        const uint64_t base = size();
        for (uint64_t b = 1; b <= n_bins; ++b) bin_off_.push_back(base + (off[b] - off[0]));
        return true;
    }

    void release()
    {
        if (keys_) munmap(keys_, cap_ * 8);
        keys_ = nullptr;
        cap_ = 0;
        bin_off_.clear();
    }

    const uint64_t *keys() const { return keys_; }
    uint64_t size() const { return bin_off_.empty() ? 0 : bin_off_.back(); }
    uint64_t bins() const { return bin_off_.empty() ? 0 : bin_off_.size() - 1; }
    const uint64_t *bin_off() const { return bin_off_.data(); }

private:
    uint64_t *keys_ = nullptr;
    uint64_t cap_ = 0;
    std::vector<uint64_t> bin_off_;
};

}
