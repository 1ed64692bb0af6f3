// plasship: rescorediagonal --rescore-mode 1 (the best local score on the candidate's diagonal, no positions) on gfx950.  Product code, built
// into the extension library libplasship_subst.so (include/plasship_ext/subst.h).  This is the filter step linclust runs on amino-acid DBs
// before its alignment (lib/mmseqs/data/workflow/linclust.sh:59-68, FILTER=1 of lib/mmseqs/src/workflow/Linclust.cpp:95,116-120): every
// k-mer candidate pair among the representatives is scanned along its diagonal; the output is a prefilter list again.
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   alignment/DistanceCalculator.h:16-38    computeSubstitutionDistance, globalAlignment = false: score = max(0, score + m[q][t]), the maximum
//   alignment/DistanceCalculator.h:93-175   computeUngappedAlignment over the diagonal's wraps (forEachWrap, asm_rules.hpp): a strictly greater
//                                           score replaces the best; the default LocalAlignment (score 0, diagonal 0, diagonalLen 0) is what
//                                           an all-non-positive pair keeps
//   alignment/rescorediagonal.cpp:193-334   canBeCovered, the coverages diagonalLen / length, seqId = alnLen = 0, the score per column, the
//                                           hit_t that is written; bit score, E-value gate and accept rule are ref_rules.hpp's
//   prefiltering/QueryMatcher.h:35-38,114-126  the diagonal is kept in an unsigned short and written as a signed short
//
// THE RECURRENCE AS A SCAN (rescore_local.hip's, without positions).  With the prefix sums P[pos] (P[-1] = 0) the score at pos is
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
// A lane's 16 columns and their scores are rescore_diag.hpp's (columnScores).  The filters are integer and IEEE float
// arithmetic on group-uniform values; the first lane of the group writes the pair's flag and line.  The host side is RescoreList (common.hpp).
// Expected bound (not separated by counters): the LDS lookups of the matrix, one byte read per column and lane, 16 KB table.  Algorithmic bytes per candidate: 16 (candidate)
// + 16 (two packed offset / length words) + 2 * overlap per wrap tried + 4 + 16 (flag, line) written, 16 per kept line copied once more.
#include "rescore_diag.hpp"
#include "../../include/plasship_ext/subst.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

namespace plasship {

struct SubstArgs {
    SeqView db;
    RescoreListArgs l;
    CandHit *lines;              // [nHits] the line of pair h in slot h (valid where keep[h])
    AcceptThr thr;
};

constexpr int SB_BLOCK = 256;
constexpr unsigned SB_PER_LANE = RD_PER_LANE;
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
        int c[SB_PER_LANE];
        columnScores(q, qLen, qo, t, to, i0, n, rev, smat, comp, c);      // (a column behind the overlap scores 0: it changes nothing)
        ScanS me; me.sum = 0; me.mn = SB_INF;
#pragma unroll
        for (unsigned j = 0; j < SB_PER_LANE; j++) { me.sum += c[j]; me.mn = min(me.mn, me.sum); }
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
// computeUngappedAlignment for RESCORE_MODE_SUBSTITUTION by a group of W lanes
template <unsigned W>
__device__ __forceinline__ SubstBest bestWrap(const PairSeqs &p, unsigned d16, const signed char *smat, const unsigned char *comp, unsigned sub) {
    SubstBest b; b.score = 0; b.diag = 0; b.diagLen = 0; b.scored = 0;
    forEachWrap(d16, p.qLen, p.tLen, [&](int real, const DiagSpan &sp) {
        const int s = scanDiagonalMax<W>(p.q, p.qLen, sp.qo, p.t, sp.to, sp.len, p.rev, smat, comp, sub);
        b.scored += sp.len;
        if (s > b.score) { b.score = s; b.diag = real; b.diagLen = sp.len; }
    });
    return b;
}

// rescorediagonal.cpp:231-332 for RESCORE_MODE_SUBSTITUTION on the best wrap: the line, and whether it is kept
__device__ __forceinline__ bool substFinish(const SubstArgs &a, const CandHit &hit, const PairSeqs &p, const SubstBest &b, CandHit &o) {
    const bool isIdentity = hit.query == hit.target;       // (one DB is query and target: sameQTDB)
    const int distance = b.score;
    const int bitScore = bitScoreOf(distance, a.l.lambda, a.l.logK, a.l.ln2);
    const float targetCov = (float) (int) b.diagLen / (float) (int) p.tLen, queryCov = (float) (int) b.diagLen / (float) (int) p.qLen;
    const bool hasEvalue = passesEvalue(distance, p.qLen, a.l.minScore, a.l.minScoreLen);
    const float scorePerCol = (float) distance / (float) (int) b.diagLen;          // (0 / 0 = NaN where nothing scored: never >= the threshold)
    o.target = hit.target; o.query = hit.query; o.prefScore = p.rev ? -bitScore : bitScore; o.diag16 = (unsigned) b.diag & 0xFFFFu;
    return acceptsPair(a.thr, isIdentity, hasEvalue, 0.0f, 0, queryCov, targetCov, scorePerCol);      // mode 1 leaves seqId = 0 and alnLen = 0
}
// the counters of the pair's owner (a group, or group 0 for the wavefront tier)
__device__ __forceinline__ void countLine(unsigned long long (&n)[RL_NSTATS], const CandHit &o, const SubstBest &b, bool kept) {
    n[RL_RESIDUES] += b.scored;
    if (kept) { n[RL_KEPT]++; if (!isImplicitSelfLine(o.query == o.target, o.prefScore, o.diag16)) n[RL_VISIBLE]++; }
}

__global__ __launch_bounds__(SB_BLOCK) void rescoreSubstKernel(SubstArgs a) {
    __shared__ signed char smat[RD_SMAT];
    __shared__ unsigned char sComp[256];
    stageTables<SB_BLOCK>(smat, sComp, a.l.mat);
    const unsigned lane = (unsigned) laneId(), grp = lane / SB_GROUP, sub = lane % SB_GROUP;
    const uint64_t wavesPerBlock = SB_BLOCK / WAVE, stride = (uint64_t) gridDim.x * wavesPerBlock * SB_PAIRS;
    unsigned long long n[RL_NSTATS] = {};      // (per group; its first lane adds them up at the end)
    for (uint64_t h0 = ((uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE) * SB_PAIRS; h0 < a.l.nHits; h0 += stride) {
        // ---- the group tier: the eight groups on their pairs, side by side ----
        const uint64_t h = h0 + grp;
        bool isLong = false;
        if (h < a.l.nHits) {
            const CandHit hit = a.l.hits[h];
            const PairSeqs p = loadPair(hit, a.l.reverseCapable, a.db);
            if (p.bad) { n[RL_BAD]++; if (sub == 0) a.l.keep[h] = 0; }
            else if (!canBeCovered(a.thr.covThr, a.thr.covMode, (float) (int) p.qLen, (float) (int) p.tLen)) { if (sub == 0) a.l.keep[h] = 0; }
            else if (min(p.qLen, p.tLen) > SB_GROUP_MAX) isLong = true;
            else {
                const SubstBest b = bestWrap<SB_GROUP>(p, hit.diag16 & 0xFFFFu, smat, sComp, sub);
                CandHit o; const bool kept = substFinish(a, hit, p, b, o);
                countLine(n, o, b, kept);
                if (sub == 0) { a.l.keep[h] = kept ? 1u : 0u; a.lines[h] = o; }
            }
        }
        // ---- the wavefront tier: the long pairs among the eight, one after the other ----
        unsigned long long longMask = __ballot(isLong && sub == 0);
        while (longMask) {
            const unsigned g = (unsigned) (__ffsll((long long) longMask) - 1) / SB_GROUP;
            longMask &= longMask - 1;
            const uint64_t hl = h0 + g;
            const CandHit hit = a.l.hits[hl];
            const PairSeqs p = loadPair(hit, a.l.reverseCapable, a.db);      // (in range: the group tier has looked)
            const SubstBest b = bestWrap<(unsigned) WAVE>(p, hit.diag16 & 0xFFFFu, smat, sComp, lane);
            CandHit o; const bool kept = substFinish(a, hit, p, b, o);
            if (lane == 0) {         // (lane 0 is the first lane of group 0: the counters of that group take the wavefront tier's)
                countLine(n, o, b, kept);
                a.l.keep[hl] = kept ? 1u : 0u; a.lines[hl] = o;
            }
        }
    }
    if (sub == 0) flushStats(a.l.stats, n);
}

}  // namespace plasship
using namespace plasship;

// subset != nullptr: the E-value's database size is the residue count of the subset's representatives (plasship_rescore_subst_subset)
static int rescoreSubst(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *subset, const plasship_subst_params *par,
                        plasship_cands **out, plasship_rescore_stats *stats, const char *what) {
    if (!ctx || !db || !c || !par || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    RescoreList rl{ctx, what, db, nullptr, c};
    if (const int rc = rl.prepare(sizeof(CandHit), false, &par->eval_thr, subset)) return rc;
    SubstArgs a; memset(&a, 0, sizeof(a));
    a.db = db->view(); a.l = rl.args; a.lines = rl.dSlots.as<CandHit>();
    a.thr.covMode = par->cov_mode; a.thr.covThr = par->cov_thr; a.thr.seqIdThr = par->seq_id_thr; a.thr.alnLenThr = par->min_aln_len;
    a.thr.filterHits = !std::isnan(par->score_per_col_thr); a.thr.scorePerColThr = a.thr.filterHits ? par->score_per_col_thr : 0.0f;
    if (a.l.nHits) {
        const uint64_t perBlock = (uint64_t) (SB_BLOCK / WAVE) * SB_PAIRS;
        const unsigned grid = (unsigned) std::min<uint64_t>((a.l.nHits + perBlock - 1) / perBlock, (uint64_t) ctx->numCU * 8);
        hipLaunchKernelGGL(rescoreSubstKernel, dim3(grid), dim3(SB_BLOCK), 0, ctx->stream, a);
    }
    std::unique_ptr<plasship_cands> holder(new plasship_cands());     // released to the caller on success only
    if (const int rc = rl.collect(holder->d_qoff, holder->d_hits, stats)) return rc;
    holder->reverseCapable = c->reverseCapable; holder->nQueries = db->n; holder->nHits = rl.nKept; holder->nNonSelf = rl.nNonSelf;
    holder->h_present = c->h_present;                                 // (a filtered list: the queries without an entry stay without one)
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
