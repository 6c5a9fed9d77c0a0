// saved_batch.h -- the host side of a batch's saved hash lists ("Search beyond device memory": capture and
// replay): the object taxor_gpu_search_take_saved hands out, the checks taxor_gpu_search_saved_begin makes before it launches
// anything, and the two figures `taxor search` decides from numbers alone -- the bound of the store from the query's size, and
// whether that bound fits.  No HIP in here: tests/sanitize/saved_batch_check.cpp runs it under ASan + UBSan.
#pragma once
#include "../../include/taxor_gpu_tools.h"

#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// All reads' hashes of one batch in batch read order, dense, with everything a replay needs beside them.  The hashes live in ONE
// pageable mapping reserved for the batch's slot bound and backed page by page as the sub-batches arrive (the KeyStore's way:
// nothing grows by copying itself); finish() gives the unused tail back.
struct taxor_gpu_saved {
    uint64_t n_reads = 0, n_bases = 0, total_hashes = 0;
    std::vector<uint32_t> read_len, n_hashes, order, sub_first;   // sub_first: n_sub_batches + 1 entries
    std::vector<uint64_t> threshold, hash_off;                    // hash_off: n_reads + 1 entries
    uint64_t *hashes = nullptr;
    uint64_t hash_cap = 0;                                        // entries the mapping holds
    // where along its read each hash lies (taxor_gpu_search_capture_positions): a second mapping managed like
    // `hashes`, 4 bytes per hash, parallel to it.  nullptr when the batch was captured without positions
    uint32_t *pos = nullptr;
    uint64_t pos_cap = 0, pos_count = 0;                          // entries the mapping holds / entries appended
    double pos_seconds = 0;                                       // seconds between the event pairs around the batch's position kernels
    uint32_t use_syncmer = 0, kmer_size = 0, syncmer_size = 0, t_syncmer = 0, scaling = 1, model = 0;
    uint64_t window_size = 0;
    double error_rate = 0, ratio = 0;

    taxor_gpu_saved() = default;
    taxor_gpu_saved(const taxor_gpu_saved &) = delete;
    taxor_gpu_saved &operator=(const taxor_gpu_saved &) = delete;
    ~taxor_gpu_saved() { release(); }

    bool reserve(uint64_t cap_hashes)
    {
        release();
        hash_cap = cap_hashes ? cap_hashes : 1;
        void *p = mmap(nullptr, hash_cap * 8, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { hash_cap = 0; return false; }
        (void)madvise(p, hash_cap * 8, MADV_HUGEPAGE);     // first-touched in 2-MiB steps where the kernel allows: the drain pays the page faults
        hashes = static_cast<uint64_t *>(p);
        total_hashes = 0;
        return true;
    }
    // the next n hashes (a sub-batch's, or a piece of one)
    bool append(const uint64_t *src, uint64_t n)
    {
        if (n > hash_cap - total_hashes) return false;
        if (n) memcpy(hashes + total_hashes, src, n * 8);
        total_hashes += n;
        return true;
    }
    // the position store beside the hashes: the same capacity in entries, reserved after reserve()
    bool reserve_positions()
    {
        release_positions();
        pos_cap = hash_cap ? hash_cap : 1;
        void *p = mmap(nullptr, pos_cap * 4, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { pos_cap = 0; return false; }
        (void)madvise(p, pos_cap * 4, MADV_HUGEPAGE);
        pos = static_cast<uint32_t *>(p);
        return true;
    }
    // the positions of the next n hashes, appended in step with append()
    bool append_positions(const uint32_t *src, uint64_t n)
    {
        if (!pos || n > pos_cap - pos_count) return false;
        if (n) memcpy(pos + pos_count, src, n * 4);
        pos_count += n;
        return true;
    }
    // the mapping shrinks to the pages that hold hashes
    void finish()
    {
        const uint64_t page = 4096, keep = ((total_hashes ? total_hashes : 1) * 8 + page - 1) / page * page;
        if (hashes && keep < hash_cap * 8) {
            munmap(reinterpret_cast<char *>(hashes) + keep, hash_cap * 8 - keep);
            hash_cap = keep / 8;
        }
        const uint64_t pkeep = ((pos_count ? pos_count : 1) * 4 + page - 1) / page * page;
        if (pos && pkeep < pos_cap * 4) {
            munmap(reinterpret_cast<char *>(pos) + pkeep, pos_cap * 4 - pkeep);
            pos_cap = pkeep / 4;
        }
    }
    void release_positions()
    {
        if (pos) munmap(pos, pos_cap * 4);
        pos = nullptr;
        pos_cap = pos_count = 0;
    }
    void release()
    {
        release_positions();
        if (hashes) munmap(hashes, hash_cap * 8);
        hashes = nullptr;
        hash_cap = total_hashes = 0;
    }
    // host bytes the object holds
    uint64_t bytes() const
    {
        return total_hashes * 8 + (pos ? pos_count * 4 : 0) + (read_len.size() + n_hashes.size() + order.size() + sub_first.size()) * 4 +
               (threshold.size() + hash_off.size()) * 8;
    }
    void view(taxor_gpu_saved_view *v) const
    {
        v->n_reads = n_reads;
        v->total_hashes = total_hashes;
        v->n_sub_batches = sub_first.empty() ? 0 : sub_first.size() - 1;
        v->read_len = read_len.data();
        v->n_hashes = n_hashes.data();
        v->threshold = threshold.data();
        v->hash_off = hash_off.data();
        v->hashes = hashes;
        v->sub_first = sub_first.data();
        v->order = order.data();
        v->use_syncmer = use_syncmer;
        v->kmer_size = kmer_size;
        v->syncmer_size = syncmer_size;
        v->t_syncmer = t_syncmer;
        v->scaling = scaling;
        v->model = model;
        v->window_size = window_size;
        v->error_rate = error_rate;
        v->ratio = ratio;
    }
};

namespace taxor {

// What the replay's copies and kernels rely on, checked on the host: "" when the saved batch is sound, else a message that names
// the field.  Offsets ascend from 0 to total_hashes and stay inside the array, n_hashes agrees with them, the sub-batches tile the
// reads, a read's place in the processing order lies inside its sub-batch.
inline std::string saved_validate(const taxor_gpu_saved &b)
{
    auto u = [](uint64_t x) { return std::to_string(x); };
    const uint64_t n = b.n_reads;
    if (n >= (1ull << 32)) return "n_reads: " + u(n) + " reads in one batch";
    if (b.read_len.size() != n || b.n_hashes.size() != n || b.threshold.size() != n || b.order.size() != n || b.hash_off.size() != n + 1)
        return "n_reads: the per-read arrays do not hold " + u(n) + " entries";
    if (b.total_hashes > b.hash_cap || (b.total_hashes && !b.hashes)) return "total_hashes: " + u(b.total_hashes) + " hashes, the array holds " + u(b.hash_cap);
    if (b.pos && (b.pos_count != b.total_hashes || b.pos_count > b.pos_cap))
        return "positions: the store holds " + u(b.pos_count) + " positions (room for " + u(b.pos_cap) + "), the batch " + u(b.total_hashes) + " hashes";
    if (b.hash_off[0] != 0) return "hash_off: the first offset is " + u(b.hash_off[0]) + ", not 0";
    for (uint64_t r = 0; r < n; ++r) {          // the offsets first, all of them: a count is judged against sound offsets
        if (b.hash_off[r + 1] < b.hash_off[r]) return "hash_off: offsets do not ascend at read " + u(r);
        if (b.hash_off[r + 1] > b.total_hashes) return "hash_off: the offset behind read " + u(r) + " lies outside the " + u(b.total_hashes) + " hashes";
    }
    for (uint64_t r = 0; r < n; ++r) {
        if (b.hash_off[r + 1] - b.hash_off[r] != b.n_hashes[r]) return "n_hashes: read " + u(r) + " has " + u(b.n_hashes[r]) + ", its offsets span " + u(b.hash_off[r + 1] - b.hash_off[r]);
        if (b.read_len[r] >= (1u << 31)) return "read_len: read " + u(r) + " is 2^31 bases or longer";
    }
    if (b.hash_off[n] != b.total_hashes) return "hash_off: the offsets end at " + u(b.hash_off[n]) + ", the array holds " + u(b.total_hashes) + " hashes";
    if (b.sub_first.empty() || b.sub_first[0] != 0 || b.sub_first.back() != n) return "sub_first: the sub-batches do not span the " + u(n) + " reads";
    for (size_t i = 0; i + 1 < b.sub_first.size(); ++i) {
        if (b.sub_first[i + 1] <= b.sub_first[i]) return "sub_first: sub-batch " + u(i) + " is empty or descends";
        const uint32_t m = b.sub_first[i + 1] - b.sub_first[i];
        for (uint32_t r = b.sub_first[i]; r < b.sub_first[i + 1]; ++r)
            if (b.order[r] >= m) return "order: entry " + u(r) + " points outside its sub-batch of " + u(m) + " reads";
    }
    return "";
}

// Minimum distance, in bases, between two open syncmers of one read.  t is the index's t_syncmer as the reference stores it: the
// 1-BASED position the minimal s-mer must take among the w = k - s + 1 s-mers of a k-mer (src/hashing/syncmer.cpp:116-142: s-mer j,
// counted from 0, stands at i - k + j + 1 and is selected at i - k + t; taxor_build.cpp:509-510 sets t = 5 at k22/s12).  Between two
// selected k-mers d bases apart either the first one's minimal s-mer has left the window (d >= t) or a smaller one has entered at the
// right end and stands at position t (d >= w - t + 1): d >= min(t, w - t + 1).  The ONE definition: the searcher sizes every read's candidate slots with it (layout_batch's hcap, whose
// violation is FLAG_CAND_OVERFLOW and which the syncmer tests sweep over every admitted k, s, t), and the saved lists' bound below
// follows from the same number.
inline int syncmer_min_gap(int k, int s, int t)
{
    const int w = k - s + 1, g = t < w - t + 1 ? t : w - t + 1;
    return g < 1 ? 1 : g;
}

// Upper bound of the distinct hashes `bases` bases of query can bring: open syncmers at most one per syncmer_min_gap bases
// (k22/s12/t5: 5), minimisers and k-mers at most one per base; a read adds at most one more, and a read with any hash has k bases.
inline uint64_t saved_hash_bound(uint64_t bases, bool use_syncmer, int k, int s, int t)
{
    const int d = use_syncmer ? syncmer_min_gap(k, s, t) : 1;
    return bases / (uint64_t)d + bases / (uint64_t)(k < 1 ? 1 : k) + 1;
}

// Host bytes the saved hash lists of a whole query may need: 8 per hash at the bound above, and per read 28 (length, count,
// processing order: 4 each; threshold and offset: 8 each) with reads at one per 200 bases, the figure the results' store is metered with.
inline uint64_t saved_bytes_bound(uint64_t bases, bool use_syncmer, int k, int s, int t)
{
    return saved_hash_bound(bases, use_syncmer, k, s, t) * 8 + (bases / 200 + 1) * 28;
}

// the store is kept when its bound and a quarter of a gibibyte beside it fit what is available (0: no figure, the running check decides)
inline bool saved_store_fits(uint64_t bound_bytes, uint64_t available_bytes)
{
    return available_bytes == 0 || (bound_bytes <= available_bytes && available_bytes - bound_bytes >= (1ull << 28));
}

} // namespace taxor
