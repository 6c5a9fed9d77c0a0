// positions_check.cpp -- the host side of `taxor search --base-positions` under ASan + UBSan: the line
// formatters that append the real base columns (taxor_amd/csrc/breakpoint_format.h, segments_format.h) with an empty id, the largest
// values, BREAK_HASH at 1 and at n - 1 and a one-hash segment -- the leading columns are the existing formatters' bytes -- and the saved
// batch's position store (taxor_amd/csrc/saved_batch.h): filled in step with the hashes, counted by bytes(), trimmed by finish(), and
// refused by name where its size is not the batch's hash count.  Prints "ok <checks>" or the first failure.
#include "saved_batch.h"
#include "segments_format.h"

#include <cstdio>
#include <string>
#include <vector>

#define CHECK(x)                                                        \
    do {                                                                \
        ++checks;                                                       \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

int main()
{
    using namespace taxor;
    uint64_t checks = 0;
    auto tabs = [](const std::string &s) { size_t n = 0; for (char c : s) n += c == '\t'; return n; };
    // ---- the headers: the existing header, two names appended
    {
        const std::string b0 = breakpoint_header(), b1 = breakpoint_header_positions(), s0 = segments_header(), s1 = segments_header_positions();
        CHECK(b1 == b0.substr(0, b0.size() - 1) + "\tLEFT_END_BASE\tBREAK_BASE\n" && tabs(b1) == 19);
        CHECK(s1 == s0.substr(0, s0.size() - 1) + "\tBASE_START\tBASE_END\n" && tabs(s1) == 20);
    }
    // ---- the breakpoint line: whatever the existing formatter writes, then the two bases
    auto bp = [&](const char *id, uint64_t id_len, uint64_t qlen, uint32_t n, uint32_t brk, uint64_t left_end, uint64_t base, const char *tail) {
        std::string old, out = "kept";
        breakpoint_line(old, id, id_len, qlen, n, 3, {"GCF_1", "562"}, 7, brk, {nullptr, "1"}, 5, 1, {"GCF_2", nullptr}, 6, 2, 4);
        breakpoint_line_positions(out, id, id_len, qlen, n, 3, {"GCF_1", "562"}, 7, brk, {nullptr, "1"}, 5, 1, {"GCF_2", nullptr}, 6, 2, 4, left_end, base);
        return out == "kept" + old.substr(0, old.size() - 1) + tail && tabs(out) == 19 && out.back() == '\n';
    };
    CHECK(bp("read 1", 6, 12000, 1200, 600, 6022, 6031, "\t6022\t6031\n"));
    CHECK(bp("", 0, 100, 9, 1, 22, 30, "\t22\t30\n"));                                            // an empty id; BREAK_HASH = 1: the first hash alone on the left
    CHECK(bp("r", 1, 100, 9, 8, 70, 78, "\t70\t78\n"));                                           // BREAK_HASH = n - 1: the last hash alone on the right
    CHECK(bp("r", 1, 100, 9, 4, 50, 10, "\t50\t10\n"));                                           // the tie rule: a position may lie in front of its neighbour's
    CHECK(bp("", 0, 18446744073709551615ull, 4294967295u, 4294967294u, 18446744073709551615ull, 18446744073709551615ull,
             "\t18446744073709551615\t18446744073709551615\n"));
    {
        std::string out;
        breakpoint_line_positions(out, "", 0, ~0ull, ~0u, ~0u, {nullptr, nullptr}, ~0u, ~0u - 1, {nullptr, nullptr}, ~0u, ~0u, {nullptr, nullptr}, ~0u, ~0u, ~0u, ~0ull, ~0ull);
        CHECK(tabs(out) == 19 && out.back() == '\n' && out.find("\t18446744073709551615\t18446744073709551615\n") != std::string::npos);
    }
    // ---- the segments line
    auto sg = [&](const char *id, uint64_t id_len, uint64_t qlen, uint32_t n, uint32_t start, uint32_t end, uint64_t b0, uint64_t b1, const char *tail) {
        std::string old, out = "kept";
        segments_line(old, id, id_len, qlen, n, 3, 3, "insert", 1100, 1000, 1, start, end, {"GCF_3", "1280"}, 180, {nullptr, nullptr}, 4);
        segments_line_positions(out, id, id_len, qlen, n, 3, 3, "insert", 1100, 1000, 1, start, end, {"GCF_3", "1280"}, 180, {nullptr, nullptr}, 4, b0, b1);
        return out == "kept" + old.substr(0, old.size() - 1) + tail && tabs(out) == 20 && out.back() == '\n';
    };
    CHECK(sg("read 1", 6, 12000, 1200, 400, 600, 4012, 6010, "\t4012\t6010\n"));
    CHECK(sg("", 0, 100, 9, 4, 5, 40, 62, "\t40\t62\n"));                                        // a one-hash segment: BASE_END = BASE_START + k
    CHECK(sg("r", 1, 100, 9, 8, 9, 78, 100, "\t78\t100\n"));                                     // the last segment may end where the read does
    CHECK(sg("", 0, 18446744073709551615ull, 2147483647u, 2147483646u, 2147483647u, 18446744073709551615ull, 18446744073709551615ull,
             "\t18446744073709551615\t18446744073709551615\n"));
    // ---- the position store of a saved batch
    {
        taxor_gpu_saved b;
        const uint64_t n = 5;
        b.n_reads = n;
        b.read_len = {100, 0, 3000, 22, 50000};
        b.n_hashes = {7, 0, 260, 1, 4100};
        b.threshold.assign(n, 1);
        b.order = {0, 1, 0, 1, 2};
        b.sub_first = {0, 2, 5};
        b.hash_off.assign(n + 1, 0);
        for (uint64_t r = 0; r < n; ++r) b.hash_off[r + 1] = b.hash_off[r] + b.n_hashes[r];
        const uint64_t total = b.hash_off[n];
        std::vector<uint64_t> h(total);
        std::vector<uint32_t> p(total);
        for (uint64_t i = 0; i < total; ++i) { h[i] = i * 0x9E3779B97F4A7C15ull; p[i] = (uint32_t)(i * 7); }
        CHECK(b.reserve(3 * total + 5000));
        CHECK(!b.append_positions(p.data(), 1));                                      // no store: refused
        const uint64_t without = b.bytes();
        CHECK(b.reserve_positions() && b.pos && b.pos_cap == b.hash_cap && b.pos_count == 0);
        for (uint64_t at = 0; at < total;) {                                          // in step with the hashes, piece by piece
            const uint64_t m = std::min<uint64_t>(total - at, 1000);
            CHECK(b.append(h.data() + at, m) && b.append_positions(p.data() + at, m));
            at += m;
        }
        CHECK(!b.append_positions(p.data(), b.pos_cap - total + 1) && b.pos_count == total);   // more than the bound: refused, nothing written
        CHECK(b.bytes() == without + total * 8 + total * 4);
        CHECK(saved_validate(b).empty());
        b.finish();
        CHECK(b.pos_cap >= total && b.pos_cap < total + 4096 / 4 + 1 && b.hash_cap >= total);
        CHECK(memcmp(b.pos, p.data(), total * 4) == 0 && memcmp(b.hashes, h.data(), total * 8) == 0);
        CHECK(saved_validate(b).empty());
        auto names = [&](const char *field) { return saved_validate(b).rfind(std::string(field) + ":", 0) == 0; };
        b.pos_count = total - 1;                                                      // a store of the wrong size, either way, by name
        CHECK(names("positions"));
        b.pos_count = total + 1;
        CHECK(names("positions"));
        b.pos_count = total;
        CHECK(saved_validate(b).empty());
        b.release_positions();                                                        // without a store the batch is sound, and smaller
        CHECK(saved_validate(b).empty() && b.pos == nullptr && b.bytes() == without + total * 8);
        CHECK(b.reserve_positions() && b.pos_count == 0);
        CHECK(total == 0 || names("positions"));                                      // present but empty
        taxor_gpu_saved_view v;
        b.view(&v);
        CHECK(v.total_hashes == total && v.hashes == b.hashes);                       // the view is what it was
    }
    {   // an empty batch with a store
        taxor_gpu_saved b;
        b.hash_off.assign(1, 0);
        b.sub_first.assign(1, 0);
        CHECK(b.reserve(0) && b.reserve_positions());
        b.finish();
        CHECK(saved_validate(b).empty() && b.bytes() == 8 + 4);
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
