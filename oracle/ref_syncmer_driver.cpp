// ref_syncmer_driver.cpp -- C entry point around the REFERENCE's syncmer selector, hashing::seq_to_syncmers
// (src/hashing/syncmer.cpp, compiled where it lies by `make ref` into oracle/_ref/libtaxor_ref_syncmer.so, with the
// reference's flags) against the stand-in headers of oracle/ref_standin/.  TEST INFRASTRUCTURE ONLY.
// With the stand-in hash being the identity, the values are the selected CANONICAL K-MERS (not their wyhash), distinct, in
// first-insertion order: the oracle's orc_seq_to_syncmers must equal orc_wyhash_u64 of them, value for value.
#include <cstddef>
#include <cstdint>

#include "syncmer.hpp"

extern "C" {

// returns the number of distinct values (may exceed cap; then out holds the first cap of them)
size_t ref_seq_to_syncmers(const char *seq, size_t len, int k, int s, int t, uint64_t *out, size_t cap)
{
    seqan3::dna5_vector v(len);
    for (size_t i = 0; i < len; ++i) v[i].assign_char(seq[i]);
    const auto set = hashing::seq_to_syncmers(k, v, s, t);
    size_t n = 0;
    for (const auto x : set) {
        if (n < cap) out[n] = (uint64_t)x;
        ++n;
    }
    return n;
}

} // extern "C"
