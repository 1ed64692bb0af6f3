// plasship: rescorediagonal --rescore-mode 0 (Hamming), with and without --wrapped-scoring, on gfx950.  Product code.
// This is linclust's Hamming pre-clustering call (lib/mmseqs/data/workflow/linclust.sh:30); the output is a prefilter list again.
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   alignment/rescorediagonal.cpp:146-356   per-hit loop for RESCORE_MODE_HAMMING: the doubled query, the reverse strand, canBeCovered, the
//                                           skipped longer target, coverage / seqId / alnLen filters, the hit_t that is written
//   alignment/DistanceCalculator.h:57-91    computeUngappedWrappedAlignment: both alias loops in unsigned arithmetic, diagonalLen
//   alignment/DistanceCalculator.h:93-175   computeUngappedAlignment / ungappedAlignmentByDiagonal: the walk without wrapping
//   alignment/DistanceCalculator.h:276-295  computeInverseHammingDistance: the number of EQUAL bytes, case-sensitive
//   commons/NucleotideMatrix.cpp:4-61       aa2num -> reverseResidue -> num2aa: the reverse strand's letters (nuclComplement, ref_rules.hpp)
//   prefiltering/QueryMatcher.h:114-126     the diagonal is written as a signed short
//
// Kernel design: ONE WAVEFRONT per candidate pair; a lane compares 16 residues per step (two unaligned 16-byte loads, one zero-byte test per
// word), the wavefront 1024, and the 64 partial counts are summed once per alias with an xor butterfly.  The doubled query of the wrapped
// mode is never built: position i of it is orig[i mod L], so the walk of an alias is split at the wrap point into two plain byte ranges
// (no mod per byte).  The reverse strand is read from the stored query backwards (16 bytes that END at the mirrored position, byte-swapped)
// and complemented through a 256-byte table in LDS.  No load reaches outside an entry: the columns behind the last full 16 are taken one
// per lane.  The filters are integer and IEEE float arithmetic on wave-uniform values; lane 0 writes the pair's flag and line.  The kept
// lines are then compacted in input order (a scan of the flags): the reference does not sort either.
// Algorithmic bytes per candidate: 12 (candidate) + 2 * diagonalLen * (aliases tried) + 12 (line written); see DESIGN.md.
#include "common.hpp"
#include "device_utils.hpp"
#include "ref_rules.hpp"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cstring>
#include <memory>

namespace plasship {

struct HammingArgs {
    SeqView q, t;
    const CandHit *hits;
    uint64_t nHits;
    uint32_t *keep;              // [nHits] 1: the pair's line is written
    CandHit *lines;              // [nHits] the line of pair h in slot h (valid where keep[h])
    int wrapped, sameDB, reverseCapable;
    int covMode; float covThr;
    float seqIdThr; int alnLenThr, seqIdMode;
    int hasEvalue;               // the Hamming E-value is 0: 0 <= -e, the same for every pair
    unsigned long long *stats;   // [0] lines kept, [1] residues compared, [2] kept lines that are not an implicit self line, [3] ids out of range
};

__device__ __forceinline__ int zeroBytes(uint32_t x) {      // exact: bit 7 of a byte of the mask is set iff the byte of x is 0
    return __popc(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu));
}

// The lane's share of the number of i < n with a[i] == b[i].  Every byte read lies in [a, a + n) or [b, b + n).
__device__ __forceinline__ int equalFwd(const char *__restrict__ a, const char *__restrict__ b, unsigned n, unsigned lane) {
    int s = 0;
    const unsigned nFull = n & ~15u;
    for (unsigned i = 16u * lane; i < nFull; i += 16u * WAVE) {
        uint32_t x[4], y[4];
        __builtin_memcpy(x, a + i, 16); __builtin_memcpy(y, b + i, 16);
#pragma unroll
        for (int k = 0; k < 4; k++) s += zeroBytes(x[k] ^ y[k]);
    }
    if (lane < n - nFull) s += (a[nFull + lane] == b[nFull + lane]) ? 1 : 0;
    return s;
}
// The same against the reverse strand: the number of i < n with comp[a[p - i]] == b[i]; requires p >= n - 1.  Every byte read lies in
// [a + p - (n - 1), a + p] or [b, b + n).
__device__ __forceinline__ int equalRev(const char *__restrict__ a, unsigned p, const char *__restrict__ b, unsigned n, unsigned lane,
                                        const unsigned char *__restrict__ comp) {
    int s = 0;
    const unsigned nFull = n & ~15u;
    for (unsigned i = 16u * lane; i < nFull; i += 16u * WAVE) {
        uint32_t v[4], y[4];
        __builtin_memcpy(v, a + (p - i - 15u), 16); __builtin_memcpy(y, b + i, 16);      // a[p-i-15 .. p-i], last byte first after the swap
        const uint32_t x[4] = {__builtin_bswap32(v[3]), __builtin_bswap32(v[2]), __builtin_bswap32(v[1]), __builtin_bswap32(v[0])};
#pragma unroll
        for (unsigned j = 0; j < 16; j++) {
            const unsigned qa = (x[j >> 2] >> (8 * (j & 3))) & 0xFFu, tb = (y[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            s += ((unsigned) comp[qa] == tb) ? 1 : 0;
        }
    }
    if (lane < n - nFull) s += ((unsigned) comp[(unsigned char) a[p - (nFull + lane)]] == (unsigned) (unsigned char) b[nFull + lane]) ? 1 : 0;
    return s;
}

constexpr int HM_BLOCK = 256;

__global__ __launch_bounds__(HM_BLOCK) void hammingKernel(HammingArgs a) {
    __shared__ unsigned char sComp[256];
    for (int i = threadIdx.x; i < 256; i += HM_BLOCK) sComp[i] = nuclComplement((unsigned char) i);
    __syncthreads();
    const unsigned lane = (unsigned) laneId();
    const uint64_t wavesPerBlock = HM_BLOCK / WAVE;
    const uint64_t stride = (uint64_t) gridDim.x * wavesPerBlock;
    unsigned long long nKept = 0, nCompared = 0, nVisible = 0, nBad = 0;      // (wave-uniform; lane 0 adds them up at the end)
    for (uint64_t h = (uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE; h < a.nHits; h += stride) {
        const CandHit hit = a.hits[h];
        const uint32_t qid = hit.query, tid = hit.target;
        if (qid >= a.q.n || tid >= a.t.n) { nBad++; if (lane == 0) a.keep[h] = 0; continue; }
        const uint64_t qv = a.q.offLen[qid], tv = a.t.offLen[tid];
        const char *q = a.q.data + (qv >> 24), *t = a.t.data + (tv >> 24);
        const unsigned L = (unsigned) qv & 0xFFFFFFu, dbLen = (unsigned) tv & 0xFFFFFFu;        // origQueryLen, dbLen
        const bool rev = a.reverseCapable && hit.prefScore < 0;
        const bool isIdentity = a.sameDB && qid == tid;
        const unsigned d16 = hit.diag16 & 0xFFFFu;
        bool kept = false;
        int32_t outScore = 0; unsigned outDiag = 0;
        // (an empty target: the reference's first wrapped loop does not end, its division by dbLen is 0 / 0 — no line is written here)
        if (dbLen > 0 && L > 0 && canBeCovered(a.covThr, a.covMode, (float) L, (float) dbLen) && !(a.wrapped && dbLen > L)) {
            unsigned best = 0, diagLen = 0; int bestDiag = 0;
            // one alias: the equal bytes of two ranges of the (possibly reversed, possibly doubled) query against the target
            //   forward: query [q0, q0 + n0) against t [t0, ..), then query [0, n1) against t [t0 + n0, ..)
            //   reverse: position j of the reverse strand is comp[q[L - 1 - j]]
            auto score = [&](unsigned q0, unsigned t0, unsigned n0, unsigned n1) -> unsigned {
                int s = rev ? equalRev(q, L - 1u - q0, t + t0, n0, lane, sComp) : equalFwd(q + q0, t + t0, n0, lane);
                if (n1) s += rev ? equalRev(q, L - 1u, t + t0 + n0, n1, lane, sComp) : equalFwd(q, t + t0 + n0, n1, lane);
                nCompared += n0 + n1;
                return (unsigned) waveReduceSum(s);
            };
            if (a.wrapped) {
                // DistanceCalculator.h:65-86: the aliases diagonal -/+ d * 65536 in unsigned arithmetic; the walk of alias r starts at position r of
                // the doubled query and covers the whole target (dbLen <= L): [r, L) and then [0, dbLen - (L - r))
                auto tryAlias = [&](unsigned r) {
                    const unsigned n0 = min(dbLen, L - r);
                    const unsigned s = score(r, 0u, n0, dbLen - n0);
                    if (s > best) { best = s; bestDiag = (int) r; }
                };
                for (unsigned d = 1; (0u - d * 65536u + d16) > (0u - dbLen); d++) tryAlias((0u - d * 65536u + d16) + L);      // in [1, L): d * 65536 - d16 < dbLen <= L
                for (unsigned d = 0; (d * 65536u + d16) < L; d++) tryAlias(d * 65536u + d16);
                diagLen = dbLen;                                        // min(dbSeqLen, querySeqLen / 2)
            } else {
                // DistanceCalculator.h:98-111,119-173: a diagonal that misses the sequences scores 0 and never wins
                for (unsigned d = 1; d <= 1u + dbLen / 32768u; d++) {
                    const int real = (int) (0u - d * 65536u + d16);
                    const unsigned dist = (unsigned) (-real);
                    if (dist >= dbLen) continue;
                    const unsigned len = min(dbLen - dist, L);
                    const unsigned s = score(0u, dist, len, 0u);
                    if (s > best) { best = s; bestDiag = real; diagLen = len; }
                }
                for (unsigned d = 0; d <= L / 65536u; d++) {
                    const unsigned dist = d * 65536u + d16;
                    if (dist >= L) continue;
                    const unsigned len = min(dbLen, L - dist);
                    const unsigned s = score(dist, 0u, len, 0u);
                    if (s > best) { best = s; bestDiag = (int) dist; diagLen = len; }
                }
            }
            // rescorediagonal.cpp:239-246,304-332
            const float targetCov = (float) diagLen / (float) dbLen, queryCov = (float) diagLen / (float) L;
            const int idCnt = (int) (float) best;
            const float seqId = computeSeqId(a.seqIdMode, idCnt, (int) L, (int) dbLen, (int) diagLen);      // (0 / 0 = NaN when no alias scored)
            const bool hasCov = hasCoverage(a.covThr, a.covMode, queryCov, targetCov);
            const bool hasSeqId = (double) seqId >= (double) (a.seqIdThr - FLT_EPSILON);
            const bool hasAlnLen = (int) diagLen >= a.alnLenThr;
            kept = isIdentity || (hasAlnLen && hasCov && hasSeqId && a.hasEvalue);
            // hit.prefScore = 100 * seqId: a double product truncated to int; what cvttsd2si makes of a NaN is INT_MIN
            const double p100 = 100.0 * (double) seqId;
            const int32_t sc = (p100 != p100 || p100 >= 2147483648.0 || p100 <= -2147483649.0) ? INT_MIN : (int32_t) p100;
            outScore = rev ? (int32_t) (0u - (uint32_t) sc) : sc;
            outDiag = (unsigned) bestDiag & 0xFFFFu;
        }
        if (kept) { nKept++; if (!(isIdentity && outScore == 0 && outDiag == 0)) nVisible++; }
        if (lane == 0) {
            a.keep[h] = kept ? 1u : 0u;
            CandHit o; o.target = tid; o.prefScore = outScore; o.diag16 = outDiag; o.query = qid;
            a.lines[h] = o;
        }
    }
    if (lane == 0) {
        if (nKept) atomicAdd(&a.stats[0], nKept);
        if (nCompared) atomicAdd(&a.stats[1], nCompared);
        if (nVisible) atomicAdd(&a.stats[2], nVisible);
        if (nBad) atomicAdd(&a.stats[3], nBad);
    }
}

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_rescore_hamming(plasship_ctx *ctx, const plasship_seqdb *qdb, const plasship_seqdb *tdb, const plasship_cands *c,
                                        const plasship_hamming_params *par, plasship_cands **out, plasship_rescore_stats *stats) {
    if (!ctx || !qdb || !tdb || !c || !par || !out) { setError("plasship_rescore_hamming: bad argument"); return PLASSHIP_ERR_ARG; }
    if (ctx->hasComm && ctx->comm.world > 1) { setError("plasship_rescore_hamming: not part of a sharded run (a communicator of more than one rank is set)"); return PLASSHIP_ERR_UNSUPPORTED; }
    if (c->nQueries != qdb->n) { setError("plasship_rescore_hamming: candidate list does not belong to the query DB"); return PLASSHIP_ERR_ARG; }
    if (qdb->dbtype != tdb->dbtype) { setError("plasship_rescore_hamming: query and target DB types differ"); return PLASSHIP_ERR_ARG; }
    const bool nucl = qdb->dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES;
    if (par->wrapped && !nucl) { setError("Wrapped scoring is only supported for nucleotides."); return PLASSHIP_ERR_ARG; }      // rescorediagonal.cpp:70-76
    if (c->reverseCapable && !nucl) { setError("plasship_rescore_hamming: a candidate list with strands on a DB that is not nucleotides"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    const uint64_t nHits = c->nHits;
    const size_t nQ = qdb->n;
    DevBuf dKeep, dLines, dStats;
    if (dKeep.alloc(std::max<uint64_t>(nHits, 1) * 4) != hipSuccess || dLines.alloc(std::max<uint64_t>(nHits, 1) * sizeof(CandHit)) != hipSuccess ||
        dStats.alloc(32) != hipSuccess) {
        setError("plasship_rescore_hamming: out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 32, ctx->stream));
    { int rcOL = ensureOffLen(ctx, qdb); if (!rcOL) rcOL = ensureOffLen(ctx, tdb); if (rcOL) return rcOL; }
    HammingArgs a; memset(&a, 0, sizeof(a));
    a.q = qdb->view(); a.t = tdb->view(); a.hits = c->d_hits.as<CandHit>(); a.nHits = nHits;
    a.keep = dKeep.as<uint32_t>(); a.lines = dLines.as<CandHit>();
    a.wrapped = par->wrapped != 0; a.sameDB = (qdb == tdb); a.reverseCapable = c->reverseCapable;
    a.covMode = par->cov_mode; a.covThr = par->cov_thr; a.seqIdThr = par->seq_id_thr; a.alnLenThr = par->min_aln_len; a.seqIdMode = par->seq_id_mode;
    a.hasEvalue = 0.0 <= par->eval_thr; a.stats = dStats.as<unsigned long long>();
    PH_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (nHits) {
        const unsigned grid = (unsigned) std::min<uint64_t>((nHits + HM_BLOCK / WAVE - 1) / (HM_BLOCK / WAVE), (uint64_t) ctx->numCU * 8);
        hipLaunchKernelGGL(hammingKernel, dim3(grid), dim3(HM_BLOCK), 0, ctx->stream, a);
    }
    PH_CHECK(hipEventRecord(ctx->ev[1], ctx->stream));
    unsigned long long hs[4] = {0, 0, 0, 0};
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hs[3]) { setError("plasship_rescore_hamming: the candidate list names sequences that are not in the DBs"); return PLASSHIP_ERR_ARG; }
    const uint64_t nKept = hs[0];
    std::unique_ptr<plasship_cands> holder(new plasship_cands());     // released to the caller on success only
    plasship_cands *o = holder.get();
    o->reverseCapable = c->reverseCapable; o->nQueries = nQ; o->nHits = nKept; o->nNonSelf = hs[2];
    // the kept lines in input order, and the CSR over them
    if (const int rc = compactCsr(ctx, "plasship_rescore_hamming", c->d_qoff.as<uint64_t>(), nQ, dLines.p, sizeof(CandHit), dKeep.as<uint32_t>(), nHits, nKept, o->d_qoff, o->d_hits)) return rc;
    if (stats) {
        stats->n_scored = nHits; stats->n_accepted = nKept; stats->overlap_residues = hs[1];
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); stats->ms_kernel = ms;
    }
    *out = holder.release();
    return PLASSHIP_OK;
}
