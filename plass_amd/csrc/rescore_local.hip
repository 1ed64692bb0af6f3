// plasship: rescorediagonal --rescore-mode 2 (the best-scoring ungapped LOCAL segment on the candidate's diagonal) on gfx950.  Product code,
// built into the extension library libplasship_linclust.so (include/plasship_ext/linclust.h).  This is linclust's alignment step when the
// workflow runs with --alignment-mode 4 (lib/mmseqs/src/workflow/Linclust.cpp:86-129: ALIGN_MODULE=rescorediagonal, --rescore-mode 2).
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   alignment/DistanceCalculator.h:93-175   computeUngappedAlignment over the diagonal's wraps (forEachWrap, asm_rules.hpp): a strictly greater
//                                           score replaces the best; the default LocalAlignment (score 0, start = end = -1, diagonal 0,
//                                           diagonalLen 0) is what an all-non-positive pair keeps
//   alignment/DistanceCalculator.h:178-201  computeSubstitutionStartEndDistance (the recurrence, below)
//   alignment/rescorediagonal.cpp:204-334   canBeCovered, alnLen, the coordinates by the diagonal's sign (alnOnDiagonal), seqId only behind the
//                                           E-value gate or for an identity pair, computeCov of the segment, the flipped query positions of
//                                           the reverse strand; bit score, E-value gate and accept rule are ref_rules.hpp's
//
// THE RECURRENCE AS A SCAN.  The reference walks pos = 0 .. len-1 with score = max(0, score + c[pos]); where the sum falls to <= 0 it
// remembers minPos = pos; a strictly greater score sets maxEndPos = pos, maxStartPos = minPos + 1.  With the prefix sums P[pos] (P[-1] = 0)
// the score at pos is P[pos] - min_{-1 <= j <= pos} P[j], minPos is the LATEST position that reaches the running minimum (ties go to the
// later position; position -1 holds the value 0), and the result is the EARLIEST position with the largest score.
//
// Kernel design: ONE WAVEFRONT per candidate pair.  A step covers 64 lanes x 16 residues: a lane fetches its 16 columns and looks their
// scores up (columnScores: rescore_diag.hpp) and forms its local (sum, minimum prefix, position of that minimum).  Six shuffle
// rounds scan the triples over the wavefront (the operator is associative: the minimum of the right part is shifted by the left part's
// sum, the right part wins ties); with the scan's value before its own residues and the carry of the steps before, a lane replays its 16
// positions sequentially, which yields its own first maximum; one butterfly picks the largest, the lower lane on ties.  The carry (prefix
// sum, running minimum and its position, best score with its start and end) is wave-uniform and goes to the next step.  Identities of
// the winning segment are counted in a second, byte-per-lane pass, only where the reference counts them.  Lane 0 writes the record and
// the keep flag; the host side is RescoreList (common.hpp).
// Overlaps of <= 64 residues take the same path (a lane-per-pair kernel for them has not been measured).
// Algorithmic bytes per candidate: 16 (candidate) + 16 (two packed offset / length words) + 2 * overlap per wrap tried + 2 * segment
// (identities) + 4 + 64 (flag, record) written, 64 per kept record copied once more; unmeasured, see DESIGN.md.
#include "rescore_diag.hpp"
#include "../../include/plasship_ext/linclust.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

namespace plasship {

struct LocalArgs {
    SeqView db;
    RescoreListArgs l;
    AlnRec *recs;                // [nHits] the record of pair h in slot h (valid where keep[h])
    AcceptThr thr; int seqIdMode;
};

constexpr int LC_BLOCK = 256;
constexpr unsigned LC_PER_LANE = RD_PER_LANE;
constexpr unsigned LC_STEP = LC_PER_LANE * WAVE;
// "no position": larger than every prefix sum (|score| <= 11, overlap < 2^24: |P| < 2^28) and small enough that a sum added to it stays an int
constexpr int LC_INF = 0x3FFFFFFF;

struct ScanT { int sum, mn, arg; };      // of a run of positions: the sum, the smallest prefix sum inside it (relative to its start), the LATEST position reaching it
__device__ __forceinline__ ScanT scanJoin(const ScanT &a, const ScanT &b) {      // a's positions come before b's
    ScanT r; r.sum = a.sum + b.sum;
    const int bm = b.mn == LC_INF ? LC_INF : a.sum + b.mn;
    const bool right = bm <= a.mn && b.mn != LC_INF;
    r.mn = right ? bm : a.mn; r.arg = right ? b.arg : a.arg;
    return r;
}

struct LocalBest { int score, start, end; };

// computeSubstitutionStartEndDistance over the overlap [0, len): query position qo + i (REV: of the reverse strand) against target position
// to + i.  Every byte read lies inside the two entries.  All lanes return the same value.
template <bool REV>
__device__ __forceinline__ LocalBest scanDiagonal(const char *__restrict__ q, unsigned qLen, unsigned qo, const char *__restrict__ t, unsigned to, unsigned len,
                                                  const signed char *__restrict__ smat, const unsigned char *__restrict__ comp, unsigned lane) {
    int carryP = 0, carryMin = 0, carryArg = -1;
    LocalBest best; best.score = 0; best.start = 0; best.end = 0;
    for (unsigned base = 0; base < len; base += LC_STEP) {
        const unsigned i0 = base + LC_PER_LANE * lane;
        const unsigned n = i0 >= len ? 0u : min(LC_PER_LANE, len - i0);
        int c[LC_PER_LANE];
        columnScores(q, qLen, qo, t, to, i0, n, REV, smat, comp, c);
        // the lane's own run
        ScanT me; me.sum = 0; me.mn = LC_INF; me.arg = 0;
#pragma unroll
        for (unsigned j = 0; j < LC_PER_LANE; j++) {
            me.sum += c[j];
            if (j < n && me.sum <= me.mn) { me.mn = me.sum; me.arg = (int) (i0 + j); }
        }
        // inclusive scan over the wavefront, then the value before the lane's own run
        ScanT inc = me;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            ScanT l; l.sum = __shfl_up(inc.sum, o, WAVE); l.mn = __shfl_up(inc.mn, o, WAVE); l.arg = __shfl_up(inc.arg, o, WAVE);
            if ((int) lane >= o) inc = scanJoin(l, inc);
        }
        ScanT ex; ex.sum = __shfl_up(inc.sum, 1, WAVE); ex.mn = __shfl_up(inc.mn, 1, WAVE); ex.arg = __shfl_up(inc.arg, 1, WAVE);
        if (lane == 0) { ex.sum = 0; ex.mn = LC_INF; ex.arg = 0; }
        int P = carryP + ex.sum, curMin = carryMin, curArg = carryArg;
        if (ex.mn != LC_INF && carryP + ex.mn <= curMin) { curMin = carryP + ex.mn; curArg = ex.arg; }
        // the lane's 16 positions, as the reference walks them
        int myScore = 0, myStart = 0, myEnd = 0;
#pragma unroll
        for (unsigned j = 0; j < LC_PER_LANE; j++) {
            P += c[j];
            if (j < n) {
                if (P <= curMin) { curMin = P; curArg = (int) (i0 + j); }
                else if (P - curMin > myScore) { myScore = P - curMin; myEnd = (int) (i0 + j); myStart = curArg + 1; }
            }
        }
        // the largest score of the step, the lower lane (the earlier position) on ties
        unsigned long long key = ((unsigned long long) (unsigned) myScore << 32) | (unsigned long long) (63u - lane);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long k2 = __shfl_xor(key, o, WAVE); key = k2 > key ? k2 : key; }
        const int win = 63 - (int) (key & 63ull);
        const int stepScore = (int) (key >> 32), stepStart = __shfl(myStart, win, WAVE), stepEnd = __shfl(myEnd, win, WAVE);
        if (stepScore > best.score) { best.score = stepScore; best.start = stepStart; best.end = stepEnd; }
        // the carry: everything up to the end of this step
        const int totSum = __shfl(inc.sum, WAVE - 1, WAVE), totMin = __shfl(inc.mn, WAVE - 1, WAVE), totArg = __shfl(inc.arg, WAVE - 1, WAVE);
        if (totMin != LC_INF && carryP + totMin <= carryMin) { carryMin = carryP + totMin; carryArg = totArg; }
        carryP += totSum;
    }
    return best;
}

// the number of i in [0, n) with (Q(qs + i) & ~0x20) == (t[ts + i] & ~0x20): rescorediagonal.cpp:277-282
template <bool REV>
__device__ __forceinline__ int countIdentities(const char *__restrict__ q, unsigned qLen, unsigned qs, const char *__restrict__ t, unsigned ts, unsigned n,
                                               const unsigned char *__restrict__ comp, unsigned lane) {
    int s = 0;
    for (unsigned i = lane; i < n; i += WAVE) {
        const unsigned a = REV ? (unsigned) comp[(unsigned char) q[qLen - 1u - (qs + i)]] : (unsigned) (unsigned char) q[qs + i];
        const unsigned b = (unsigned) (unsigned char) t[ts + i];
        s += ((a & ~0x20u) == (b & ~0x20u)) ? 1 : 0;
    }
    return waveReduceSum(s);
}

__global__ __launch_bounds__(LC_BLOCK) void rescoreLocalKernel(LocalArgs a) {
    __shared__ signed char smat[RD_SMAT];
    __shared__ unsigned char sComp[256];
    stageTables<LC_BLOCK>(smat, sComp, a.l.mat);
    const unsigned lane = (unsigned) laneId();
    const uint64_t wavesPerBlock = LC_BLOCK / WAVE, stride = (uint64_t) gridDim.x * wavesPerBlock;
    unsigned long long n[RL_NSTATS] = {};      // (wave-uniform; lane 0 adds them up at the end)
    for (uint64_t h = (uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE; h < a.l.nHits; h += stride) {
        const CandHit hit = a.l.hits[h];
        const PairSeqs p = loadPair(hit, a.l.reverseCapable, a.db);
        if (p.bad) { n[RL_BAD]++; if (lane == 0) a.l.keep[h] = 0; continue; }
        const char *q = p.q, *t = p.t;
        const unsigned qLen = p.qLen, tLen = p.tLen;
        const bool isReverse = p.rev;
        const bool isIdentity = hit.query == hit.target;     // (one DB is query and target: sameQTDB)
        AlnRec rec; memset(&rec, 0, sizeof(rec));
        rec.query = hit.query; rec.target = hit.target;
        bool kept = false;
        if (canBeCovered(a.thr.covThr, a.thr.covMode, (float) qLen, (float) tLen)) {
            int bScore = 0, bStart = -1, bEnd = -1, bDiag = 0; unsigned bDiagLen = 0;
            forEachWrap(hit.diag16 & 0xFFFFu, qLen, tLen, [&](int real, const DiagSpan &sp) {
                const LocalBest s = isReverse ? scanDiagonal<true>(q, qLen, sp.qo, t, sp.to, sp.len, smat, sComp, lane) : scanDiagonal<false>(q, qLen, sp.qo, t, sp.to, sp.len, smat, sComp, lane);
                n[RL_RESIDUES] += sp.len;
                if (s.score > bScore) { bScore = s.score; bStart = s.start; bEnd = s.end; bDiag = real; bDiagLen = sp.len; }
            });
            // ---- wave-uniform finish (rescorediagonal.cpp:231-314) ----
            const int distance = bScore;
            const int alnLen = (bEnd - bStart) + 1;
            const AlnCoords co = alnOnDiagonal(bDiag, bStart, bEnd);
            int qS = co.qStart, qE = co.qEnd; const int dS = co.dbStart, dE = co.dbEnd;
            const bool hasEvalue = passesEvalue(distance, qLen, a.l.minScore, a.l.minScoreLen);
            float seqId = 0.0f;
            if (hasEvalue || isIdentity) {
                // (no diagonal scored > 0: the reference's identity loop runs over the single index -1 of both strings; for the identity pair
                //  both bytes are the same byte — the rule of the mode 3 kernel, rescore.hip.  On the REVERSE strand the reference reads the
                //  byte before two different buffers there, which is undefined: the 1 below is this build's choice, not a restatement;
                //  the case needs an -e that admits score 0)
                int idCnt;
                if (bStart < 0) idCnt = isIdentity ? 1 : 0;
                else idCnt = isReverse ? countIdentities<true>(q, qLen, (unsigned) qS, t, (unsigned) dS, (unsigned) alnLen, sComp, lane)
                                       : countIdentities<false>(q, qLen, (unsigned) qS, t, (unsigned) dS, (unsigned) alnLen, sComp, lane);
                seqId = computeSeqId(a.seqIdMode, idCnt, (int) qLen, (int) tLen, alnLen);
            }
            const float queryCov = computeCov((unsigned) qS, (unsigned) qE, qLen);
            const float targetCov = computeCov((unsigned) dS, (unsigned) dE, tLen);
            if (isReverse) { qS = (int) qLen - qS - 1; qE = (int) qLen - qE - 1; }
            const float scorePerCol = (float) distance / (float) (int) bDiagLen;      // (0 / 0 = NaN where nothing scored: never >= the threshold)
            kept = acceptsPair(a.thr, isIdentity, hasEvalue, seqId, alnLen, queryCov, targetCov, scorePerCol);
            rec.bitScore = bitScoreOf(distance, a.l.lambda, a.l.logK, a.l.ln2); rec.rawScore = distance; rec.seqId = seqId;
            rec.qStart = qS; rec.qEnd = qE; rec.qLen = (int) qLen; rec.dbStart = dS; rec.dbEnd = dE; rec.dbLen = (int) tLen;
            rec.alnLen = alnLen; rec.reversed = isReverse ? 1 : 0;
        }
        rec.accepted = kept ? 1 : 0; rec.btKind = 1;           // ungapped: the backtrace is one run of alnLen 'M'
        if (kept) n[RL_KEPT]++;
        if (lane == 0) { a.l.keep[h] = kept ? 1u : 0u; a.recs[h] = rec; }
    }
    if (lane == 0) flushStats(a.l.stats, n);
}

}  // namespace plasship
using namespace plasship;

// subset != nullptr: the E-value's database size is the residue count of the subset's representatives (plasship_rescore_local_subset)
static int rescoreLocal(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *subset, const plasship_local_params *par,
                        plasship_alns **out, plasship_rescore_stats *stats, const char *what) {
    if (!ctx || !db || !c || !par || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    RescoreList rl{ctx, what, db, nullptr, c};
    if (const int rc = rl.prepare(sizeof(AlnRec), false, &par->eval_thr, subset)) return rc;
    LocalArgs a; memset(&a, 0, sizeof(a));
    a.db = db->view(); a.l = rl.args; a.recs = rl.dSlots.as<AlnRec>();
    a.thr.covMode = par->cov_mode; a.thr.covThr = par->cov_thr; a.thr.seqIdThr = par->seq_id_thr; a.thr.alnLenThr = par->min_aln_len; a.seqIdMode = par->seq_id_mode;
    a.thr.filterHits = !std::isnan(par->score_per_col_thr); a.thr.scorePerColThr = a.thr.filterHits ? par->score_per_col_thr : 0.0f;
    if (a.l.nHits) {
        const unsigned grid = (unsigned) std::min<uint64_t>((a.l.nHits + LC_BLOCK / WAVE - 1) / (LC_BLOCK / WAVE), (uint64_t) ctx->numCU * 8);
        hipLaunchKernelGGL(rescoreLocalKernel, dim3(grid), dim3(LC_BLOCK), 0, ctx->stream, a);
    }
    std::unique_ptr<plasship_alns> holder(new plasship_alns());     // released to the caller on success only
    plasship_alns *al = holder.get();
    if (const int rc = rl.collect(al->d_qoff, al->d_recs, stats)) return rc;
    al->nQueries = db->n; al->nucl = rl.nucl; al->addBacktrace = par->add_backtrace != 0; al->dbResidues = rl.residues;
    al->nLines = rl.nKept; al->nSlots = rl.nKept; al->sparse = false; al->selfPending = false; al->qdb = db; al->tdb = db;
    *out = holder.release();
    return PLASSHIP_OK;
}

extern "C" int plasship_rescore_local(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_local_params *par,
                                      plasship_alns **out, plasship_rescore_stats *stats) {
    return rescoreLocal(ctx, db, c, nullptr, par, out, stats, "plasship_rescore_local");
}

extern "C" int plasship_rescore_local_subset(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *cl,
                                             const plasship_local_params *par, plasship_alns **out, plasship_rescore_stats *stats) {
    if (!cl) { setError("plasship_rescore_local_subset: bad argument"); return PLASSHIP_ERR_ARG; }
    return rescoreLocal(ctx, db, c, cl, par, out, stats, "plasship_rescore_local_subset");
}
