// Device code that only the list-in, list-out rescore kernels share (rescore_hamming.hip: mode 0, rescore_subst.hip: mode 1,
// rescore_local.hip: mode 2): the LDS tables of a block, a lane's 16 columns of one diagonal, the counters of a launch.  The pair rules
// are in ref_rules.hpp, the walk over a diagonal's wraps in asm_rules.hpp; the scans over the columns differ on purpose and stay with
// their kernels.
#pragma once
#include "common.hpp"
#include "device_utils.hpp"
#include "ref_rules.hpp"
#include "asm_rules.hpp"

namespace plasship {

constexpr unsigned RD_PER_LANE = 16;             // columns a lane takes per step
constexpr int RD_SMAT = 128 * 128;               // the matrix in LDS: row stride 128, rows and columns 123 .. 127 are 0: the index of a column is (a & 127) << 7 | (b & 127)

// ---- the block prologue.  The reverse strand is never built: it is read backwards from the stored query and complemented through a
// 256-byte table in LDS (nuclComplement, ref_rules.hpp).  Both functions end with the block's barrier. ----
template <int BLOCK> __device__ __forceinline__ void stageComplement(unsigned char (&sComp)[256]) {
    for (int i = threadIdx.x; i < 256; i += BLOCK) sComp[i] = nuclComplement((unsigned char) i);
    __syncthreads();
}
// mat: the 123 x 123 ASCII-indexed matrix in global memory
template <int BLOCK> __device__ __forceinline__ void stageTables(signed char (&smat)[RD_SMAT], unsigned char (&sComp)[256], const signed char *__restrict__ mat) {
    for (int i = threadIdx.x; i < RD_SMAT; i += BLOCK) smat[i] = ((i & 127) < 123 && (i >> 7) < 123) ? mat[(i >> 7) * 123 + (i & 127)] : (signed char) 0;
    stageComplement<BLOCK>(sComp);
}

// ---- a lane's 16 columns ----
// the 16 stored bytes that END at `last`, last byte first: 16 letters of the reverse strand, before the complement
__device__ __forceinline__ void load16Rev(const char *__restrict__ last, uint32_t (&x)[4]) {
    uint32_t v[4]; __builtin_memcpy(v, last - 15u, 16);
    x[0] = __builtin_bswap32(v[3]); x[1] = __builtin_bswap32(v[2]); x[2] = __builtin_bswap32(v[1]); x[3] = __builtin_bswap32(v[0]);
}
// The scores of columns [i0, i0 + n) of the overlap (n <= 16): m[Q(qo + i)][t[to + i]] from the LDS tables, Q the stored query or (rev) its
// reverse strand; 0 behind n.  The fetch: sixteen columns are two unaligned 16-byte loads; the lane that holds the end of the overlap
// reads it byte by byte, so no load leaves the two entries.  (The fetched bytes stay inside this function: handed to the caller as two
// byte arrays they cost the mode 2 kernel 6 VGPRs and its fourth wavefront per SIMD.)
__device__ __forceinline__ void columnScores(const char *__restrict__ q, unsigned qLen, unsigned qo, const char *__restrict__ t, unsigned to, unsigned i0, unsigned n,
                                             bool rev, const signed char *__restrict__ smat, const unsigned char *__restrict__ comp, int (&c)[RD_PER_LANE]) {
    unsigned char qa[RD_PER_LANE], tb[RD_PER_LANE];
    if (n == RD_PER_LANE) {
        uint32_t y[4]; __builtin_memcpy(y, t + to + i0, 16);
        uint32_t x[4];
        if (rev) load16Rev(q + (qLen - 1u - (qo + i0)), x);
        else __builtin_memcpy(x, q + qo + i0, 16);
#pragma unroll
        for (unsigned j = 0; j < RD_PER_LANE; j++) { qa[j] = (unsigned char) (x[j >> 2] >> (8 * (j & 3))); tb[j] = (unsigned char) (y[j >> 2] >> (8 * (j & 3))); }
    } else {
#pragma unroll
        for (unsigned j = 0; j < RD_PER_LANE; j++) {
            const bool in = j < n;
            qa[j] = in ? (unsigned char) (rev ? q[qLen - 1u - (qo + i0 + j)] : q[qo + i0 + j]) : (unsigned char) 0;
            tb[j] = in ? (unsigned char) t[to + i0 + j] : (unsigned char) 0;
        }
    }
#pragma unroll
    for (unsigned j = 0; j < RD_PER_LANE; j++) {
        const unsigned a = rev ? (unsigned) comp[qa[j]] : (unsigned) qa[j];
        c[j] = j < n ? (int) smat[((a & 127u) << 7) | (tb[j] & 127u)] : 0;
    }
}

// ---- the counters of a launch (RescoreStat, common.hpp): kept by whoever owns a pair (a wavefront, or an eight-lane group) and added up
// by its first lane at the end ----
__device__ __forceinline__ void flushStats(unsigned long long *stats, const unsigned long long (&n)[RL_NSTATS]) {
#pragma unroll
    for (int k = 0; k < RL_NSTATS; k++) if (n[k]) atomicAdd(&stats[k], n[k]);
}

}  // namespace plasship
