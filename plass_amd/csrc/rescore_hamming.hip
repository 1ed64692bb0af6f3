// plasship: rescorediagonal --rescore-mode 0 (Hamming), with and without --wrapped-scoring, on gfx950.  Product code.
// This is linclust's Hamming pre-clustering call (lib/mmseqs/data/workflow/linclust.sh:30); the output is a prefilter list again.
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   alignment/rescorediagonal.cpp:146-356   per-hit loop for RESCORE_MODE_HAMMING: the doubled query, the reverse strand, canBeCovered, the
//                                           skipped longer target, coverage / seqId / alnLen filters, the hit_t that is written
//   alignment/DistanceCalculator.h:57-91    computeUngappedWrappedAlignment: both alias loops in unsigned arithmetic, diagonalLen
//   alignment/DistanceCalculator.h:93-175   computeUngappedAlignment / ungappedAlignmentByDiagonal: the walk without wrapping (forEachWrap)
//   alignment/DistanceCalculator.h:276-295  computeInverseHammingDistance: the number of EQUAL bytes, case-sensitive
//   prefiltering/QueryMatcher.h:114-126     the diagonal is written as a signed short
//
// Kernel design: ONE WAVEFRONT per candidate pair; a lane compares 16 residues per step (two unaligned 16-byte loads, one zero-byte test per
// word), the wavefront 1024, and the 64 partial counts are summed once per alias with an xor butterfly.  The doubled query of the wrapped
// mode is never built: position i of it is orig[i mod L], so the walk of an alias is split at the wrap point into two plain byte ranges
// (no mod per byte).  No load reaches outside an entry: the columns behind the last full 16 are taken one per lane.  The filters are
// integer and IEEE float arithmetic on wave-uniform values; lane 0 writes the pair's flag and line.  What this kernel shares with modes
// 1 and 2 — the pair, the accept rule, the reverse strand's table and fetch, the counters, the host side — is in ref_rules.hpp,
// rescore_diag.hpp and RescoreList (common.hpp).
// Algorithmic bytes per candidate: 12 (candidate) + 2 * diagonalLen * (aliases tried) + 12 (line written); see DESIGN.md.
#include "rescore_diag.hpp"
#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>

namespace plasship {

struct HammingArgs {
    SeqView q, t;
    RescoreListArgs l;
    CandHit *lines;              // [nHits] the line of pair h in slot h (valid where keep[h])
    int wrapped, sameDB;
    AcceptThr thr; int seqIdMode;
    int hasEvalue;               // the Hamming E-value is 0: 0 <= -e, the same for every pair
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
        uint32_t x[4], y[4];
        load16Rev(a + (p - i), x); __builtin_memcpy(y, b + i, 16);
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
    stageComplement<HM_BLOCK>(sComp);
    const unsigned lane = (unsigned) laneId();
    const uint64_t wavesPerBlock = HM_BLOCK / WAVE;
    const uint64_t stride = (uint64_t) gridDim.x * wavesPerBlock;
    unsigned long long n[RL_NSTATS] = {};      // (wave-uniform; lane 0 adds them up at the end)
    for (uint64_t h = (uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE; h < a.l.nHits; h += stride) {
        const CandHit hit = a.l.hits[h];
        const PairSeqs p = loadPair(hit, a.l.reverseCapable, a.q, a.t);
        if (p.bad) { n[RL_BAD]++; if (lane == 0) a.l.keep[h] = 0; continue; }
        const char *q = p.q, *t = p.t;
        const unsigned L = p.qLen, dbLen = p.tLen;        // origQueryLen, dbLen
        const bool rev = p.rev;
        const bool isIdentity = a.sameDB && hit.query == hit.target;
        const unsigned d16 = hit.diag16 & 0xFFFFu;
        bool kept = false;
        int32_t outScore = 0; unsigned outDiag = 0;
        // (an empty target: the reference's first wrapped loop does not end, its division by dbLen is 0 / 0 — no line is written here)
        if (dbLen > 0 && L > 0 && canBeCovered(a.thr.covThr, a.thr.covMode, (float) L, (float) dbLen) && !(a.wrapped && dbLen > L)) {
            unsigned best = 0, diagLen = 0; int bestDiag = 0;
            // one alias: the equal bytes of two ranges of the (possibly reversed, possibly doubled) query against the target
            //   forward: query [q0, q0 + n0) against t [t0, ..), then query [0, n1) against t [t0 + n0, ..)
            //   reverse: position j of the reverse strand is comp[q[L - 1 - j]]
            auto score = [&](unsigned q0, unsigned t0, unsigned n0, unsigned n1) -> unsigned {
                int s = rev ? equalRev(q, L - 1u - q0, t + t0, n0, lane, sComp) : equalFwd(q + q0, t + t0, n0, lane);
                if (n1) s += rev ? equalRev(q, L - 1u, t + t0 + n0, n1, lane, sComp) : equalFwd(q, t + t0 + n0, n1, lane);
                n[RL_RESIDUES] += n0 + n1;
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
                forEachWrap(d16, L, dbLen, [&](int real, const DiagSpan &sp) {
                    const unsigned s = score(sp.qo, sp.to, sp.len, 0u);
                    if (s > best) { best = s; bestDiag = real; diagLen = sp.len; }
                });
            }
            // rescorediagonal.cpp:239-246,304-332
            const float targetCov = (float) diagLen / (float) dbLen, queryCov = (float) diagLen / (float) L;
            const int idCnt = (int) (float) best;
            const float seqId = computeSeqId(a.seqIdMode, idCnt, (int) L, (int) dbLen, (int) diagLen);      // (0 / 0 = NaN when no alias scored)
            kept = acceptsPair(a.thr, isIdentity, a.hasEvalue, seqId, (int) diagLen, queryCov, targetCov, 0.0f);
            // hit.prefScore = 100 * seqId: a double product truncated to int; what cvttsd2si makes of a NaN is INT_MIN
            const double p100 = 100.0 * (double) seqId;
            const int32_t sc = (p100 != p100 || p100 >= 2147483648.0 || p100 <= -2147483649.0) ? INT_MIN : (int32_t) p100;
            outScore = rev ? (int32_t) (0u - (uint32_t) sc) : sc;
            outDiag = (unsigned) bestDiag & 0xFFFFu;
        }
        if (kept) { n[RL_KEPT]++; if (!isImplicitSelfLine(isIdentity, outScore, outDiag)) n[RL_VISIBLE]++; }
        if (lane == 0) {
            a.l.keep[h] = kept ? 1u : 0u;
            CandHit o; o.target = hit.target; o.prefScore = outScore; o.diag16 = outDiag; o.query = hit.query;
            a.lines[h] = o;
        }
    }
    if (lane == 0) flushStats(a.l.stats, n);
}

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_rescore_hamming(plasship_ctx *ctx, const plasship_seqdb *qdb, const plasship_seqdb *tdb, const plasship_cands *c,
                                        const plasship_hamming_params *par, plasship_cands **out, plasship_rescore_stats *stats) {
    if (!ctx || !qdb || !tdb || !c || !par || !out) { setError("plasship_rescore_hamming: bad argument"); return PLASSHIP_ERR_ARG; }
    RescoreList rl{ctx, "plasship_rescore_hamming", qdb, tdb, c};
    if (const int rc = rl.prepare(sizeof(CandHit), par->wrapped != 0, nullptr, nullptr)) return rc;
    HammingArgs a; memset(&a, 0, sizeof(a));
    a.q = qdb->view(); a.t = tdb->view(); a.l = rl.args; a.lines = rl.dSlots.as<CandHit>();
    a.wrapped = par->wrapped != 0; a.sameDB = (qdb == tdb);
    a.thr.covMode = par->cov_mode; a.thr.covThr = par->cov_thr; a.thr.seqIdThr = par->seq_id_thr; a.thr.alnLenThr = par->min_aln_len; a.seqIdMode = par->seq_id_mode;
    a.hasEvalue = 0.0 <= par->eval_thr;
    if (a.l.nHits) {
        const unsigned grid = (unsigned) std::min<uint64_t>((a.l.nHits + HM_BLOCK / WAVE - 1) / (HM_BLOCK / WAVE), (uint64_t) ctx->numCU * 8);
        hipLaunchKernelGGL(hammingKernel, dim3(grid), dim3(HM_BLOCK), 0, ctx->stream, a);
    }
    std::unique_ptr<plasship_cands> holder(new plasship_cands());     // released to the caller on success only
    if (const int rc = rl.collect(holder->d_qoff, holder->d_hits, stats)) return rc;
    holder->reverseCapable = c->reverseCapable; holder->nQueries = qdb->n; holder->nHits = rl.nKept; holder->nNonSelf = rl.nNonSelf;
    *out = holder.release();
    return PLASSHIP_OK;
}
