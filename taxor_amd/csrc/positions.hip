// positions.hip -- where along its read each saved hash lies (taxor_gpu_search_capture_positions).
//
//   k_hash_positions   pos[i] = min { p in [0, L-k] : wyhash_u64(canon(f_p)) == hashes[i] }  for every hash of a sub-batch's dense
//                      lists, f_p the k-mer at base p of the PACKED read (after the dna4 mapping), canon the smaller of it and its
//                      reverse complement.  Syncmer lists only: their values are wyhash(canonical k-mer) and they are deduplicated.
//
// One block per read (grid-stride).  The read's list is taken in pieces of at most POS_PIECE consecutive hashes: a piece goes into an
// open-addressing table in LDS (8-byte key + one word that is EMPTY, or the smallest position seen so far), the block sweeps all
// L - k + 1 k-mer starts in tiles of POS_TILE -- words staged as k_syncmers stages sW, one canonical k-mer, one wyhash and one probe
// per start, an LDS atomicMin on a match -- and the piece's hashes then look themselves up again and store their word.  A read with P
// pieces is swept P times.  The kernel writes EVERY entry of every list, the sentinel included where no k-mer matched (which the
// host reports as an internal error): the output needs no preset.  No block waits on another; every loop runs to a given count.
#include "kernels.h"
#include "device_prims.h"
#include "ixf_arith.h"

namespace taxor {

static constexpr int POS_BLK = 512;
static constexpr int POS_PIECE = 2048;                 // hashes per piece
static constexpr int POS_TAB = 4096;                   // slots: a load of at most one half
static constexpr int POS_TILE = 4096;                  // k-mer starts per staged tile
static constexpr int POS_WORDS = POS_TILE / 16 + 3;    // a start in the tile's last word reads two words past it (k <= 32)
static constexpr uint32_t POS_EMPTY = 0xFFFFFFFFu;     // a free slot
static constexpr uint32_t POS_UNSEEN = 0xFFFFFFFEu;    // a slot whose hash no k-mer has matched yet (positions are < 2^31)
// 32 KiB of keys + 16 KiB of words + 1 KiB of staged bases: three blocks of eight waves per CU (160 KiB of LDS)

// the slot function of the syncmer kernels' dedup (kernels.hip dedup_slot)
__device__ __forceinline__ uint32_t pos_slot(uint64_t h, uint32_t mask)
{
    h ^= h >> 31;
    h *= 0x9E3779B97F4A7C15ull;
    return (uint32_t)(h >> 32) & mask;
}

__global__ __launch_bounds__(POS_BLK) void k_hash_positions(const uint32_t *__restrict__ packed, const uint64_t *__restrict__ poff,
                                                            const uint32_t *__restrict__ rlen, const uint64_t *__restrict__ off,
                                                            const uint64_t *__restrict__ dense, uint32_t *__restrict__ pos, uint64_t dense_cap,
                                                            uint32_t n_reads, int k)
{
    __shared__ uint64_t sKey[POS_TAB];
    __shared__ uint32_t sMin[POS_TAB];
    __shared__ uint32_t sW[POS_WORDS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t o0 = off[r], o1 = off[r + 1];
        if (o1 <= o0 || o1 > dense_cap) continue;           // no hash; or a list the gather left out (the host sees off[n] > dense_cap)
        const uint64_t cnt = o1 - o0;
        const uint32_t L = rlen[r];
        const uint32_t *__restrict__ pk = packed + poff[r];
        const uint32_t nwords = (((L + 15u) >> 4) + 3u) & ~3u;   // reads start on a 4-word boundary and are padded to one (k_pack_dna4)
        const uint32_t nwin = L >= (uint32_t)k ? L - (uint32_t)k + 1u : 0u;
        for (uint64_t p0 = 0; p0 < cnt; p0 += POS_PIECE) {
            const uint32_t pn = cnt - p0 < (uint64_t)POS_PIECE ? (uint32_t)(cnt - p0) : (uint32_t)POS_PIECE;
            // the smallest power of two that keeps the load at one half or below: a short read clears and probes a short table
            uint32_t slots = 64;
            while (slots < 2u * pn) slots <<= 1;            // <= POS_TAB, since pn <= POS_PIECE
            const uint32_t mask = slots - 1u;
            __syncthreads();                                // the piece (or read) before is done with the table
            for (uint32_t q = tid; q < slots; q += POS_BLK) sMin[q] = POS_EMPTY;
            __syncthreads();
            // ---- the piece's hashes take their slots (they are distinct: the lists are deduplicated) --------------------------
            for (uint32_t i = tid; i < pn; i += POS_BLK) {
                const uint64_t h = dense[o0 + p0 + i];
                uint32_t q = pos_slot(h, mask);
                for (uint32_t step = 0; step < slots; ++step) {
                    if (atomicCAS(&sMin[q], POS_EMPTY, POS_UNSEEN) == POS_EMPTY) { sKey[q] = h; break; }
                    q = (q + 1u) & mask;
                }
            }
            // ---- sweep the read's k-mer starts ---------------------------------------------------------------------------------
            for (uint32_t x0 = 0; x0 < nwin; x0 += POS_TILE) {
                __syncthreads();                            // keys are in place / the tile before has been read
                const uint32_t wbase = x0 >> 4;
                if (tid < (uint32_t)POS_WORDS) {
                    const uint32_t wi = wbase + tid;
                    sW[tid] = wi < nwords ? pk[wi] : 0u;
                }
                __syncthreads();
                const uint32_t nt = min((uint32_t)POS_TILE, nwin - x0);
                for (uint32_t j = tid; j < nt; j += POS_BLK) {
                    const uint32_t x = x0 + j;
                    const uint64_t h = wyhash_u64(canon(lds_bases(sW, (x >> 4) - wbase, x & 15u, k), k));   // syncmer.cpp:144-145
                    uint32_t q = pos_slot(h, mask);
                    for (uint32_t step = 0; step < slots; ++step) {
                        const uint32_t v = sMin[q];
                        if (v == POS_EMPTY) break;
                        if (sKey[q] == h) {
                            if (x < v) atomicMin(&sMin[q], x);
                            break;
                        }
                        q = (q + 1u) & mask;
                    }
                }
            }
            __syncthreads();
            // ---- every hash of the piece finds its slot again and stores its word ------------------------------------------------
            for (uint32_t i = tid; i < pn; i += POS_BLK) {
                const uint64_t h = dense[o0 + p0 + i];
                uint32_t q = pos_slot(h, mask), out = POS_EMPTY;
                for (uint32_t step = 0; step < slots; ++step) {
                    const uint32_t v = sMin[q];
                    if (v == POS_EMPTY) break;
                    if (sKey[q] == h) {
                        out = v == POS_UNSEEN ? POS_EMPTY : v;
                        break;
                    }
                    q = (q + 1u) & mask;
                }
                pos[o0 + p0 + i] = out;
            }
        }
    }
}

void launch_hash_positions(const uint32_t *packed, const uint64_t *poff, const uint32_t *rlen, const uint64_t *off, const uint64_t *dense,
                           uint32_t *pos, uint64_t dense_cap, uint32_t n_reads, int k, hipStream_t st)
{
    if (!n_reads) return;
    const uint32_t grid = n_reads < 8192u ? n_reads : 8192u;
    hipLaunchKernelGGL(k_hash_positions, dim3(grid), dim3(POS_BLK), 0, st, packed, poff, rlen, off, dense, pos, dense_cap, n_reads, k);
}

} // namespace taxor
