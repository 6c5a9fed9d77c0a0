// fastx_scan.h -- library-internal interface of the device record scanner (fastx_scan.hip), used by api.hip.
#pragma once
#include "kernels.h"

#include <stdint.h>

namespace taxor {

struct FastxScan;                       // device scratch and host tables of one searcher's scanner

struct FastxTable {
    uint64_t n_reads;
    const uint64_t *id_off, *id_len, *read_len;   // host arrays, valid until the next scan with the same FastxScan
    uint32_t status;                    // 0 or TAXOR_FASTX_IRREGULAR
};

FastxScan *fastx_scan_create();
void fastx_scan_destroy(FastxScan *fx);

// Records of d_raw[0, n_bytes) (device memory; kind '>' or '@'; last_byte = the buffer's last byte, which the host holds) -> their
// table.  Synchronises st.  Nothing but the scanner's own scratch is written.
int fastx_scan_records(FastxScan *fx, const uint8_t *d_raw, uint64_t n_bytes, int kind, uint8_t last_byte, hipStream_t st, FastxTable *out);

// The reads of the last scan, packed 2 bits per base at packed + poff[r] (k_pack_dna4's layout: the words of a read padded to a
// multiple of four).  A byte outside dna15 raises FLAG_ALPHABET in ctr.  Asynchronous on st.
int fastx_scan_pack(FastxScan *fx, const uint8_t *d_raw, const uint64_t *d_poff, const uint32_t *d_rlen, uint32_t *d_packed,
                    uint64_t n_reads, Counters *ctr, hipStream_t st);

}   // namespace taxor
