// saved_batch_check.cpp -- the host side of a batch's saved hash lists (taxor_amd/csrc/saved_batch.h) under ASan + UBSan: the store
// takes a batch's hashes piece by piece and gives its unused tail back, the view shows what went in, every way of breaking what a
// replay relies on is refused with the field's name, and the store's bound and the keep-or-re-read decision answer from numbers.
// Prints "ok <checks>" or the first failure.
#include "saved_batch.h"

#include <cinttypes>
#include <random>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

static void fill(taxor_gpu_saved &b, std::mt19937_64 &rng, uint64_t n, uint32_t per_sub)
{
    b.n_reads = n;
    b.read_len.assign(n, 0);
    b.n_hashes.assign(n, 0);
    b.threshold.assign(n, 0);
    b.order.assign(n, 0);
    b.hash_off.assign(n + 1, 0);
    b.sub_first.assign(1, 0);
    for (uint64_t r = 0; r < n; ++r) {
        b.n_hashes[r] = r % 7 == 0 ? 0 : (uint32_t)(rng() % 300);
        b.read_len[r] = b.n_hashes[r] * 11 + 22;
        b.threshold[r] = b.n_hashes[r] / 3;
        b.hash_off[r + 1] = b.hash_off[r] + b.n_hashes[r];
        if ((r + 1) % per_sub == 0 || r + 1 == n) b.sub_first.push_back((uint32_t)(r + 1));
    }
    for (size_t i = 0; i + 1 < b.sub_first.size(); ++i)
        for (uint32_t r = b.sub_first[i]; r < b.sub_first[i + 1]; ++r) b.order[r] = b.sub_first[i + 1] - 1 - r;      // a permutation: reversed
}

int main()
{
    using namespace taxor;
    uint64_t checks = 0;
    std::mt19937_64 rng(11);
    // ---- the store: reserved for a slot bound, filled in pieces, shrunk to what it holds
    {
        taxor_gpu_saved b;
        fill(b, rng, 1000, 96);
        const uint64_t total = b.hash_off[1000];
        std::vector<uint64_t> all(total);
        for (auto &x : all) x = rng();
        CHECK(b.reserve(3 * total + 100000));
        for (uint64_t at = 0; at < total;) {
            const uint64_t n = std::min<uint64_t>(total - at, 1 + rng() % 5000);
            CHECK(b.append(all.data() + at, n));
            at += n;
        }
        CHECK(b.total_hashes == total);
        CHECK(!b.append(all.data(), b.hash_cap - total + 1));          // more than the bound: refused, nothing written
        CHECK(b.total_hashes == total);
        b.finish();
        CHECK(b.hash_cap >= total && b.hash_cap < total + 4096 / 8 + 1);
        CHECK(memcmp(b.hashes, all.data(), total * 8) == 0);
        CHECK(saved_validate(b).empty());
        taxor_gpu_saved_view v{};
        b.view(&v);
        CHECK(v.n_reads == 1000 && v.total_hashes == total && v.n_sub_batches == b.sub_first.size() - 1 && v.hashes == b.hashes);
        CHECK(v.hash_off[1000] == total && v.sub_first[v.n_sub_batches] == 1000);
        CHECK(b.bytes() == total * 8 + (3 * 1000 + b.sub_first.size()) * 4 + (1000 + 1001) * 8);
        // ---- what a replay relies on, broken one field at a time
        auto names = [&](const char *field) { return saved_validate(b).rfind(std::string(field) + ":", 0) == 0; };
        { const uint64_t k = b.hash_off[500]; b.hash_off[500] = b.hash_off[499] - 1; CHECK(names("hash_off")); b.hash_off[500] = k; }
        { const uint64_t k = b.hash_off[1000]; b.hash_off[1000] = total + 1; CHECK(names("hash_off")); b.hash_off[1000] = k; }
        { const uint64_t k = b.hash_off[0]; b.hash_off[0] = 1; CHECK(names("hash_off")); b.hash_off[0] = k; }
        { b.n_hashes[3] += 1; CHECK(names("n_hashes")); b.n_hashes[3] -= 1; }
        { b.read_len[9] = 1u << 31; CHECK(names("read_len")); b.read_len[9] = 22; }
        { b.sub_first.back() = 999; CHECK(names("sub_first")); b.sub_first.back() = 1000; }
        { const uint32_t k = b.sub_first[2]; b.sub_first[2] = b.sub_first[1]; CHECK(names("sub_first")); b.sub_first[2] = k; }
        { b.order[100] = 96; CHECK(names("order")); b.order[100] = b.sub_first[2] - 1 - 100; }
        { b.threshold.pop_back(); CHECK(names("n_reads")); b.threshold.push_back(0); }
        { const uint64_t k = b.total_hashes; b.total_hashes = b.hash_cap + 1; CHECK(names("total_hashes")); b.total_hashes = k; }
        CHECK(saved_validate(b).empty());
    }
    // ---- a batch without reads, and one whose reads have no hashes
    {
        taxor_gpu_saved b;
        fill(b, rng, 0, 8);
        CHECK(b.reserve(0));
        b.finish();
        CHECK(saved_validate(b).empty());
        taxor_gpu_saved c;
        fill(c, rng, 1, 8);
        CHECK(c.n_hashes[0] == 0 && c.reserve(64));
        c.finish();
        CHECK(saved_validate(c).empty() && c.bytes() == 4 * 4 + 3 * 8 + 4);
    }
    // ---- the bound and the decision
    {
        CHECK(saved_hash_bound(0, true, 22, 12, 5) == 1);
        CHECK(saved_hash_bound(1100000, true, 22, 12, 5) == 1100000 / 5 + 1100000 / 22 + 1);           // k22/s12/t5: one hash per 5 bases
        CHECK(saved_hash_bound(1000, true, 28, 20, 4) == 1000 / 4 + 1000 / 28 + 1);
        CHECK(saved_hash_bound(1000, true, 32, 31, 1) == 1000 + 1000 / 32 + 1);
        CHECK(saved_hash_bound(1000, false, 20, 0, 0) == 1000 + 50 + 1);                               // minimisers: one per base
        CHECK(saved_bytes_bound(2000, true, 22, 12, 5) == (400 + 90 + 1) * 8 + 11 * 28);
        CHECK(saved_bytes_bound(~0ull >> 8, false, 20, 0, 0) > (~0ull >> 8));                          // (no overflow below 2^56 bases)
        CHECK(saved_store_fits(1ull << 30, 0));                                                          // no figure: the running check decides
        CHECK(saved_store_fits(1ull << 30, (1ull << 30) + (1ull << 28)));
        CHECK(!saved_store_fits(1ull << 30, (1ull << 30) + (1ull << 28) - 1));
        CHECK(!saved_store_fits(1ull << 30, 1ull << 20));
        CHECK(saved_store_fits(0, 1ull << 28) && !saved_store_fits(0, (1ull << 28) - 1));
    }
    printf("ok %" PRIu64 "\n", checks);
    return 0;
}
