// plasship: rescorediagonal --rescore-mode 1 (the best local score on the candidate's diagonal, no positions) on gfx950.  Product code, built
// into the extension library libplasship_subst.so (include/plasship_ext/subst.h).  This is the filter step linclust runs on amino-acid DBs
// before its alignment (lib/mmseqs/data/workflow/linclust.sh:59-68, FILTER=1 of lib/mmseqs/src/workflow/Linclust.cpp:95,116-120): every
// k-mer candidate pair among the representatives is scanned along its diagonal; the output is a prefilter list again.
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   alignment/DistanceCalculator.h:16-38    computeSubstitutionDistance, globalAlignment = false: score = max(0, score + m[q][t]), the maximum
//   alignment/DistanceCalculator.h:93-113   computeUngappedAlignment: the wraps d - 65536 j (j = 1 .. 1 + dbLen / 32768), then d + 65536 j
//                                           (j = 0 .. qLen / 65536), a strictly greater score replaces the best; the default LocalAlignment
//                                           (score 0, diagonal 0, diagonalLen 0) is what an all-non-positive pair keeps
//   alignment/DistanceCalculator.h:115-175  the overlap of one diagonal
//   alignment/rescorediagonal.cpp:193-334   canBeCovered, the coverages diagonalLen / length, E-value and bit score, seqId = alnLen = 0, the
//                                           score per column (0 / 0 = NaN where nothing scored), the accept rule, the hit_t that is written
//   prefiltering/QueryMatcher.h:35-38,114-126  the diagonal is kept in an unsigned short and written as a signed short
//
// THE RECURRENCE AS A SCAN (rescore_local.hip:15-32 without positions).  With the prefix sums P[pos] (P[-1] = 0) the score at pos is
// P[pos] - min_{-1 <= j <= pos} P[j], and only its maximum is wanted: no position, no tie rule, no identity pass.  A column of score 0 never
// changes the maximum (P stays, the minimum stays), so the columns behind the end of an overlap are padded with 0 and no lane needs a count.
// The scan element of a run of columns is (sum, smallest prefix sum inside it); a lane scans its 16 columns, the group scans the lanes'
// elements, and with the value before its own columns and the carry of the steps before, a lane replays its 16 columns for its own
// maximum; one reduction takes the largest.
//
// Kernel design: TWO TIERS in one kernel.  A wavefront takes eight consecutive pairs.  A pair whose shorter sequence has at most
// SB_GROUP_MAX = 1024 residues — every overlap of it fits one step of a wavefront, which would leave lanes idle — is scanned by ONE EIGHT-LANE
// GROUP (the precedent: assembleresults' groups for short queues) in steps of 8 lanes x 16 residues; the eight groups of the wavefront
// work on their pairs side by side, the scan of the group is three DPP row shifts and the maximum three DPP steps, all on the VALU.
// The longer pairs among the eight are then taken one after the other by the WHOLE WAVEFRONT in steps of 64 lanes x 16 residues (six shuffle
// rounds, as in the mode 2 kernel).  Protein overlaps are a few hundred residues: two to four steps of a group.  The hand-over was
// chosen, not swept; what was measured (the group tier on 49-residue fragments: 0.33 ns per pair) is in DESIGN.md.
// A lane loads its 16 residues of both sequences with two unaligned 16-byte loads; the lane that holds the end of the overlap reads it
// byte by byte — no load leaves the entry.  The reverse strand is read backwards from the stored query and complemented through the
// 256-byte LDS table (nuclComplement, ref_rules.hpp), like the other rescore kernels do.  The filters are integer and IEEE float arithmetic
// on group-uniform values; the first lane of the group writes the pair's flag and line.  The kept lines are compacted in input order.
// Expected bound (not separated by counters): the LDS lookups of the matrix, one byte read per column and lane, 16 KB table.  Algorithmic bytes per candidate: 16 (candidate)
// + 16 (two packed offset / length words) + 2 * overlap per wrap tried + 4 + 16 (flag, line) written, 16 per kept line copied once more.
#include "common.hpp"
#include "../../include/plasship_ext/subst.h"
#include "device_utils.hpp"
#include "host_util.hpp"
#include "ref_rules.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

namespace plasship {

struct SubstArgs {
    SeqView db;
    const CandHit *hits;
    uint64_t nHits;
    uint32_t *keep;              // [nHits] 1: the pair's line is written
    CandHit *lines;              // [nHits] the line of pair h in slot h (valid where keep[h])
    const uint32_t *minScore;    // [minScoreLen] the smallest raw score that passes -e for that query length
    uint32_t minScoreLen;
    const signed char *mat;      // 123 x 123 in global memory, staged to LDS
    int reverseCapable;
    int covMode; float covThr;
    float seqIdThr; int alnLenThr;
    int filterHits; float scorePerColThr;
    double lambda, logK, ln2;
    unsigned long long *stats;   // [0] lines kept, [1] residues scored, [2] kept lines that are not an implicit self line, [3] ids out of range
};

constexpr int SB_BLOCK = 256;
constexpr unsigned SB_PER_LANE = 16;
constexpr unsigned SB_GROUP = 8;                 // lanes of a group; a wavefront holds WAVE / SB_GROUP pairs
constexpr unsigned SB_PAIRS = WAVE / SB_GROUP;
constexpr unsigned SB_GROUP_MAX = 1024;          // min(qLen, tLen) <= this: the group tier (one step of the wavefront tier covers as much)
// "no prefix": larger than every prefix sum (|score| <= 11, overlap < 2^24: |P| < 2^28) and small enough that a sum added to it stays an int
constexpr int SB_INF = 0x3FFFFFFF;

struct ScanS { int sum, mn; };                   // of a run of columns: the sum, the smallest prefix sum inside it (relative to its start)

// the scan over the W lanes of a group (W = 8: DPP row shifts, a value that comes from another group is never used; W = 64: shuffles):
// inc = the element of all columns of the group up to and including the lane's, ex = up to the lane's, tot = of the whole group
template <unsigned W> __device__ __forceinline__ void groupScan(const ScanS me, unsigned sub, ScanS &ex, ScanS &tot);
template <> __device__ __forceinline__ void groupScan<SB_GROUP>(const ScanS me, unsigned sub, ScanS &ex, ScanS &tot) {
    ScanS inc = me;
#define SB_ROUND(o, CTRL) { const int ls = (int) dppMov<CTRL>((uint32_t) inc.sum), lm = (int) dppMov<CTRL>((uint32_t) inc.mn); \
                            if (sub >= o) { inc.mn = min(lm, ls + inc.mn); inc.sum += ls; } }
    SB_ROUND(1u, 0x111) SB_ROUND(2u, 0x112) SB_ROUND(4u, 0x114)                 // row_shr:1, 2, 4
#undef SB_ROUND
    ex.sum = (int) dppMov<0x111>((uint32_t) inc.sum); ex.mn = (int) dppMov<0x111>((uint32_t) inc.mn);
    if (sub == 0) { ex.sum = 0; ex.mn = SB_INF; }
    const int last = laneId() | (int) (SB_GROUP - 1);
    tot.sum = __shfl(inc.sum, last, WAVE); tot.mn = __shfl(inc.mn, last, WAVE);
}
template <> __device__ __forceinline__ void groupScan<(unsigned) WAVE>(const ScanS me, unsigned sub, ScanS &ex, ScanS &tot) {
    ScanS inc = me;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int ls = __shfl_up(inc.sum, o, WAVE), lm = __shfl_up(inc.mn, o, WAVE);
        if ((int) sub >= o) { inc.mn = min(lm, ls + inc.mn); inc.sum += ls; }
    }
    ex.sum = __shfl_up(inc.sum, 1, WAVE); ex.mn = __shfl_up(inc.mn, 1, WAVE);
    if (sub == 0) { ex.sum = 0; ex.mn = SB_INF; }
    tot.sum = __shfl(inc.sum, WAVE - 1, WAVE); tot.mn = __shfl(inc.mn, WAVE - 1, WAVE);
}
template <unsigned W> __device__ __forceinline__ int groupMax(int v);
template <> __device__ __forceinline__ int groupMax<SB_GROUP>(int v) {           // xor 1, xor 2, mirror inside the eight lanes
    v = max(v, (int) dppMov<0xB1>((uint32_t) v)); v = max(v, (int) dppMov<0x4E>((uint32_t) v)); v = max(v, (int) dppMov<0x141>((uint32_t) v));
    return v;
}
template <> __device__ __forceinline__ int groupMax<(unsigned) WAVE>(int v) { return waveReduceMax(v); }

// computeSubstitutionDistance over the overlap [0, len): query position qo + i (rev: of the reverse strand) against target position to + i,
// by a group of W lanes (sub: the lane's index in it).  Every byte read lies inside the two entries.  All lanes of the group return the
// same value.
template <unsigned W>
__device__ __forceinline__ int scanDiagonalMax(const char *__restrict__ q, unsigned qLen, unsigned qo, const char *__restrict__ t, unsigned to, unsigned len, bool rev,
                                               const signed char *__restrict__ smat, const unsigned char *__restrict__ comp, unsigned sub) {
    int carryP = 0, carryMin = 0, best = 0;
    for (unsigned base = 0; base < len; base += SB_PER_LANE * W) {
        const unsigned i0 = base + SB_PER_LANE * sub;
        const unsigned n = i0 >= len ? 0u : min(SB_PER_LANE, len - i0);
        unsigned char qa[SB_PER_LANE], tb[SB_PER_LANE];
        if (n == SB_PER_LANE) {
            uint32_t y[4]; __builtin_memcpy(y, t + to + i0, 16);
            uint32_t x[4];
            if (rev) {      // the 16 stored bytes that END at the mirrored position, last byte first
                uint32_t v[4]; __builtin_memcpy(v, q + (qLen - 1u - (qo + i0)) - 15u, 16);
                x[0] = __builtin_bswap32(v[3]); x[1] = __builtin_bswap32(v[2]); x[2] = __builtin_bswap32(v[1]); x[3] = __builtin_bswap32(v[0]);
            } else __builtin_memcpy(x, q + qo + i0, 16);
#pragma unroll
            for (unsigned j = 0; j < SB_PER_LANE; j++) { qa[j] = (unsigned char) (x[j >> 2] >> (8 * (j & 3))); tb[j] = (unsigned char) (y[j >> 2] >> (8 * (j & 3))); }
        } else {
#pragma unroll
            for (unsigned j = 0; j < SB_PER_LANE; j++) {
                const bool in = j < n;
                qa[j] = in ? (unsigned char) (rev ? q[qLen - 1u - (qo + i0 + j)] : q[qo + i0 + j]) : (unsigned char) 0;
                tb[j] = in ? (unsigned char) t[to + i0 + j] : (unsigned char) 0;
            }
        }
        int c[SB_PER_LANE];
        ScanS me; me.sum = 0; me.mn = SB_INF;
#pragma unroll
        for (unsigned j = 0; j < SB_PER_LANE; j++) {
            const unsigned a = rev ? (unsigned) comp[qa[j]] : (unsigned) qa[j];
            c[j] = j < n ? (int) smat[((a & 127u) << 7) | (tb[j] & 127u)] : 0;      // (a column behind the overlap scores 0: it changes nothing)
            me.sum += c[j]; me.mn = min(me.mn, me.sum);
        }
        ScanS ex, tot;
        groupScan<W>(me, sub, ex, tot);
        int P = carryP + ex.sum, curMin = min(carryMin, carryP + ex.mn), mine = 0;
#pragma unroll
        for (unsigned j = 0; j < SB_PER_LANE; j++) { P += c[j]; curMin = min(curMin, P); mine = max(mine, P - curMin); }
        best = max(best, groupMax<W>(mine));
        carryMin = min(carryMin, carryP + tot.mn); carryP += tot.sum;
    }
    return best;
}

struct SubstBest { int score, diag; unsigned diagLen; unsigned long long scored; };
// computeUngappedAlignment for RESCORE_MODE_SUBSTITUTION by a group of W lanes (DistanceCalculator.h:98-111,119-173: a wrap that misses the
// sequences scores 0 and never wins)
template <unsigned W>
__device__ __forceinline__ SubstBest bestWrap(const char *q, unsigned qLen, const char *t, unsigned tLen, unsigned d16, bool rev,
                                              const signed char *smat, const unsigned char *comp, unsigned sub) {
    SubstBest b; b.score = 0; b.diag = 0; b.diagLen = 0; b.scored = 0;
    for (unsigned d = 1; d <= 1u + tLen / 32768u; d++) {
        const unsigned dist = d * 65536u - d16;
        if (dist >= tLen) continue;
        const unsigned len = min(tLen - dist, qLen);
        const int s = scanDiagonalMax<W>(q, qLen, 0u, t, dist, len, rev, smat, comp, sub);
        b.scored += len;
        if (s > b.score) { b.score = s; b.diag = -(int) dist; b.diagLen = len; }
    }
    for (unsigned d = 0; d <= qLen / 65536u; d++) {
        const unsigned dist = d * 65536u + d16;
        if (dist >= qLen) continue;
        const unsigned len = min(tLen, qLen - dist);
        const int s = scanDiagonalMax<W>(q, qLen, dist, t, 0u, len, rev, smat, comp, sub);
        b.scored += len;
        if (s > b.score) { b.score = s; b.diag = (int) dist; b.diagLen = len; }
    }
    return b;
}

// rescorediagonal.cpp:231-332 for RESCORE_MODE_SUBSTITUTION on the best wrap: the line, and whether it is kept
__device__ __forceinline__ bool substFinish(const SubstArgs &a, const CandHit &hit, unsigned qLen, unsigned tLen, bool rev, const SubstBest &b, CandHit &o) {
    const bool isIdentity = hit.query == hit.target;       // (one DB is query and target: sameQTDB)
    const int distance = b.score;
    const int bitScore = (int) (fma(a.lambda, (double) distance, -a.logK) / a.ln2 + 0.5);
    const float targetCov = (float) (int) b.diagLen / (float) (int) tLen, queryCov = (float) (int) b.diagLen / (float) (int) qLen;
    const uint32_t ms = (qLen < a.minScoreLen) ? a.minScore[qLen] : 0xFFFFFFFFu;
    const bool hasEvalue = (uint32_t) distance >= ms;
    const float scorePerCol = (float) distance / (float) (int) b.diagLen;          // (0 / 0 = NaN where nothing scored: never >= the threshold)
    const bool hasCov = hasCoverage(a.covThr, a.covMode, queryCov, targetCov);
    const bool hasSeqId = 0.0 >= (double) (a.seqIdThr - FLT_EPSILON);               // mode 1 leaves seqId = 0
    const bool hasAlnLen = 0 >= a.alnLenThr;                                        // and alnLen = 0
    const bool hasToFilter = a.filterHits && scorePerCol >= a.scorePerColThr;
    o.target = hit.target; o.query = hit.query; o.prefScore = rev ? -bitScore : bitScore; o.diag16 = (unsigned) b.diag & 0xFFFFu;
    return isIdentity || hasToFilter || (hasAlnLen && hasCov && hasSeqId && hasEvalue);
}

__global__ __launch_bounds__(SB_BLOCK) void rescoreSubstKernel(SubstArgs a) {
    __shared__ signed char smat[128 * 128];              // row stride 128, rows and columns 123 .. 127 are 0: the index of a column is (a & 127) << 7 | (b & 127)
    __shared__ unsigned char sComp[256];
    for (int i = threadIdx.x; i < 128 * 128; i += SB_BLOCK) smat[i] = ((i & 127) < 123 && (i >> 7) < 123) ? a.mat[(i >> 7) * 123 + (i & 127)] : (signed char) 0;
    for (int i = threadIdx.x; i < 256; i += SB_BLOCK) sComp[i] = nuclComplement((unsigned char) i);
    __syncthreads();
    const unsigned lane = (unsigned) laneId(), grp = lane / SB_GROUP, sub = lane % SB_GROUP;
    const uint64_t wavesPerBlock = SB_BLOCK / WAVE, stride = (uint64_t) gridDim.x * wavesPerBlock * SB_PAIRS;
    unsigned long long nKept = 0, nScored = 0, nVisible = 0, nBad = 0;      // (per group; its first lane adds them up at the end)
    for (uint64_t h0 = ((uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE) * SB_PAIRS; h0 < a.nHits; h0 += stride) {
        // ---- the group tier: the eight groups on their pairs, side by side ----
        const uint64_t h = h0 + grp;
        bool isLong = false;
        if (h < a.nHits) {
            const CandHit hit = a.hits[h];
            if (hit.query >= a.db.n || hit.target >= a.db.n) { nBad++; if (sub == 0) a.keep[h] = 0; }
            else {
                const uint64_t qv = a.db.offLen[hit.query], tv = a.db.offLen[hit.target];
                const unsigned qLen = (unsigned) qv & 0xFFFFFFu, tLen = (unsigned) tv & 0xFFFFFFu;
                if (!canBeCovered(a.covThr, a.covMode, (float) (int) qLen, (float) (int) tLen)) { if (sub == 0) a.keep[h] = 0; }
                else if (min(qLen, tLen) > SB_GROUP_MAX) isLong = true;
                else {
                    const bool rev = a.reverseCapable && hit.prefScore < 0;
                    const SubstBest b = bestWrap<SB_GROUP>(a.db.data + (qv >> 24), qLen, a.db.data + (tv >> 24), tLen, hit.diag16 & 0xFFFFu, rev, smat, sComp, sub);
                    CandHit o; const bool kept = substFinish(a, hit, qLen, tLen, rev, b, o);
                    nScored += b.scored;
                    if (kept) { nKept++; if (!(hit.query == hit.target && o.prefScore == 0 && o.diag16 == 0)) nVisible++; }
                    if (sub == 0) { a.keep[h] = kept ? 1u : 0u; a.lines[h] = o; }
                }
            }
        }
        // ---- the wavefront tier: the long pairs among the eight, one after the other ----
        unsigned long long longMask = __ballot(isLong && sub == 0);
        while (longMask) {
            const unsigned g = (unsigned) (__ffsll((long long) longMask) - 1) / SB_GROUP;
            longMask &= longMask - 1;
            const uint64_t hl = h0 + g;
            const CandHit hit = a.hits[hl];
            const uint64_t qv = a.db.offLen[hit.query], tv = a.db.offLen[hit.target];
            const unsigned qLen = (unsigned) qv & 0xFFFFFFu, tLen = (unsigned) tv & 0xFFFFFFu;
            const bool rev = a.reverseCapable && hit.prefScore < 0;
            const SubstBest b = bestWrap<(unsigned) WAVE>(a.db.data + (qv >> 24), qLen, a.db.data + (tv >> 24), tLen, hit.diag16 & 0xFFFFu, rev, smat, sComp, lane);
            CandHit o; const bool kept = substFinish(a, hit, qLen, tLen, rev, b, o);
            if (lane == 0) {         // (lane 0 is the first lane of group 0: the counters of that group take the wavefront tier's)
                nScored += b.scored;
                if (kept) { nKept++; if (!(hit.query == hit.target && o.prefScore == 0 && o.diag16 == 0)) nVisible++; }
                a.keep[hl] = kept ? 1u : 0u; a.lines[hl] = o;
            }
        }
    }
    if (sub == 0) {
        if (nKept) atomicAdd(&a.stats[0], nKept);
        if (nScored) atomicAdd(&a.stats[1], nScored);
        if (nVisible) atomicAdd(&a.stats[2], nVisible);
        if (nBad) atomicAdd(&a.stats[3], nBad);
    }
}

}  // namespace plasship
using namespace plasship;

// subset != nullptr: the E-value's database size is the residue count of the subset's representatives (plasship_rescore_subst_subset)
static int rescoreSubst(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *subset, const plasship_subst_params *par,
                        plasship_cands **out, plasship_rescore_stats *stats, const char *what) {
    if (!ctx || !db || !c || !par || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (ctx->hasComm && ctx->comm.world > 1) { setError(std::string(what) + ": not part of a sharded run (a communicator of more than one rank is set)"); return PLASSHIP_ERR_UNSUPPORTED; }
    if (c->nQueries != db->n) { setError(std::string(what) + ": candidate list does not belong to the DB"); return PLASSHIP_ERR_ARG; }
    const bool nucl = db->dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES;
    if (c->reverseCapable && !nucl) { setError(std::string(what) + ": a candidate list with strands on a DB that is not nucleotides"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    const uint64_t nHits = c->nHits;
    const size_t nQ = db->n;
    // the E-value gate as a per-query-length minimum score (exact: E(score) is monotone; host_util.cpp), for the lengths the DB holds
    const uint32_t maxQLen = db->maxEntryLen >= 2 ? db->maxEntryLen - 2 : 0;
    const uint32_t tabLen = maxQLen + 1;
    std::vector<uint32_t> lens(nQ), minScore(tabLen, 0xFFFFFFFFu);
    PH_CHECK(plasship::streamSync(ctx->stream));
    if (nQ) { const int rc = stagedCopyToHost(ctx, lens.data(), db->d_len.p, nQ * 4); if (rc) return rc; }
    uint64_t residues = db->residues;
    if (subset) {
        if (subset->n != db->n || subset->dbGen != db->gen) { setError(std::string(what) + ": the clustering does not belong to this DB"); return PLASSHIP_ERR_ARG; }
        std::vector<uint32_t> repOf(nQ);
        if (nQ) { const int rc = stagedCopyToHost(ctx, repOf.data(), subset->d_repOf.p, nQ * 4); if (rc) return rc; }
        residues = 0;
        for (size_t q = 0; q < nQ; q++) if (repOf[q] == q) residues += lens[q];
    }
    HostEvaluer ev(nucl, residues);
    {
        std::vector<uint8_t> present(tabLen, 0);
        for (uint32_t l : lens) if (l < tabLen) present[l] = 1;
        const int maxEntry = nucl ? 2 : 11;               // the largest matrix entry: an overlap of l columns scores at most maxEntry * l
        int guess = -1;
        for (uint32_t l = 1; l < tabLen; l++)
            if (present[l]) { guess = ev.minScoreForEvalue(par->eval_thr, (int) l, maxEntry * (int) l + 1, guess); minScore[l] = (uint32_t) guess; }
    }
    DevBuf dKeep, dLines, dStats, dMinScore, dMat;
    if (dKeep.alloc(std::max<uint64_t>(nHits, 1) * 4) != hipSuccess || dLines.alloc(std::max<uint64_t>(nHits, 1) * sizeof(CandHit)) != hipSuccess ||
        dStats.alloc(32) != hipSuccess || dMinScore.alloc((size_t) tabLen * 4) != hipSuccess || dMat.alloc(123 * 123) != hipSuccess) {
        setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 32, ctx->stream));
    { const int rc = stagedCopyToDevice(ctx, dMinScore.p, minScore.data(), (uint64_t) tabLen * 4); if (rc) return rc; }
    { const int rc = stagedCopyToDevice(ctx, dMat.p, asciiSubMat(nucl), 123 * 123); if (rc) return rc; }
    { const int rc = ensureOffLen(ctx, db); if (rc) return rc; }
    SubstArgs a; memset(&a, 0, sizeof(a));
    a.db = db->view(); a.hits = c->d_hits.as<CandHit>(); a.nHits = nHits; a.keep = dKeep.as<uint32_t>(); a.lines = dLines.as<CandHit>();
    a.minScore = dMinScore.as<uint32_t>(); a.minScoreLen = tabLen; a.mat = dMat.as<signed char>(); a.reverseCapable = c->reverseCapable;
    a.covMode = par->cov_mode; a.covThr = par->cov_thr; a.seqIdThr = par->seq_id_thr; a.alnLenThr = par->min_aln_len;
    a.filterHits = !std::isnan(par->score_per_col_thr); a.scorePerColThr = a.filterHits ? par->score_per_col_thr : 0.0f;
    a.lambda = ev.g[0]; a.logK = ev.logK; a.ln2 = ev.ln2; a.stats = dStats.as<unsigned long long>();
    PH_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (nHits) {
        const uint64_t perBlock = (uint64_t) (SB_BLOCK / WAVE) * SB_PAIRS;
        const unsigned grid = (unsigned) std::min<uint64_t>((nHits + perBlock - 1) / perBlock, (uint64_t) ctx->numCU * 8);
        hipLaunchKernelGGL(rescoreSubstKernel, dim3(grid), dim3(SB_BLOCK), 0, ctx->stream, a);
    }
    PH_CHECK(hipEventRecord(ctx->ev[1], ctx->stream));
    unsigned long long hs[4] = {0, 0, 0, 0};
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hs[3]) { setError(std::string(what) + ": the candidate list names sequences that are not in the DB"); return PLASSHIP_ERR_ARG; }
    const uint64_t nKept = hs[0];
    std::unique_ptr<plasship_cands> holder(new plasship_cands());     // released to the caller on success only
    plasship_cands *o = holder.get();
    o->reverseCapable = c->reverseCapable; o->nQueries = nQ; o->nHits = nKept; o->nNonSelf = hs[2];
    o->h_present = c->h_present;                                      // (a filtered list: the queries without an entry stay without one)
    // the kept lines in input order, and the CSR over them
    if (const int rc = compactCsr(ctx, what, c->d_qoff.as<uint64_t>(), nQ, dLines.p, sizeof(CandHit), dKeep.as<uint32_t>(), nHits, nKept, o->d_qoff, o->d_hits)) return rc;
    if (stats) {
        stats->n_scored = nHits; stats->n_accepted = nKept; stats->overlap_residues = hs[1];
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); stats->ms_kernel = ms;
    }
    *out = holder.release();
    return PLASSHIP_OK;
}

extern "C" int plasship_rescore_subst(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_subst_params *par,
                                      plasship_cands **out, plasship_rescore_stats *stats) {
    return rescoreSubst(ctx, db, c, nullptr, par, out, stats, "plasship_rescore_subst");
}

extern "C" int plasship_rescore_subst_subset(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *cl,
                                             const plasship_subst_params *par, plasship_cands **out, plasship_rescore_stats *stats) {
    if (!cl) { setError("plasship_rescore_subst_subset: bad argument"); return PLASSHIP_ERR_ARG; }
    return rescoreSubst(ctx, db, c, cl, par, out, stats, "plasship_rescore_subst_subset");
}
