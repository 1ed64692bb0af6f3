// plasship: rescorediagonal --rescore-mode 2 (the best-scoring ungapped LOCAL segment on the candidate's diagonal) on gfx950.  Product code,
// built into the extension library libplasship_linclust.so (include/plasship_ext/linclust.h).  This is linclust's alignment step when the
// workflow runs with --alignment-mode 4 (lib/mmseqs/src/workflow/Linclust.cpp:86-129: ALIGN_MODULE=rescorediagonal, --rescore-mode 2).
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   alignment/DistanceCalculator.h:93-113   computeUngappedAlignment: the wraps d - 65536 j (j = 1 .. 1 + dbLen / 32768), then d + 65536 j
//                                           (j = 0 .. qLen / 65536), a strictly greater score replaces the best; the default LocalAlignment
//                                           (score 0, start = end = -1, diagonal 0, diagonalLen 0) is what an all-non-positive pair keeps
//   alignment/DistanceCalculator.h:115-175  the overlap of one diagonal
//   alignment/DistanceCalculator.h:178-201  computeSubstitutionStartEndDistance (the recurrence, below)
//   alignment/rescorediagonal.cpp:204-334   canBeCovered, alnLen, the coordinates by the diagonal's sign, E-value and bit score, seqId only
//                                           behind the E-value gate or for an identity pair, computeCov of the segment, the flipped query
//                                           positions of the reverse strand, hasToFilter, the accept rule
//
// THE RECURRENCE AS A SCAN.  The reference walks pos = 0 .. len-1 with score = max(0, score + c[pos]); where the sum falls to <= 0 it
// remembers minPos = pos; a strictly greater score sets maxEndPos = pos, maxStartPos = minPos + 1.  With the prefix sums P[pos] (P[-1] = 0)
// the score at pos is P[pos] - min_{-1 <= j <= pos} P[j], minPos is the LATEST position that reaches the running minimum (ties go to the
// later position; position -1 holds the value 0), and the result is the EARLIEST position with the largest score.
//
// Kernel design: ONE WAVEFRONT per candidate pair.  A step covers 64 lanes x 16 residues: a lane loads its 16 residues of both sequences
// (two unaligned 16-byte loads; the lane that holds the end of the overlap reads it byte by byte — no load leaves the entry), looks the 16
// scores up in the LDS copy of the ASCII-indexed matrix and forms its local (sum, minimum prefix, position of that minimum).  Six shuffle
// rounds scan the triples over the wavefront (the operator is associative: the minimum of the right part is shifted by the left part's
// sum, the right part wins ties); with the scan's value before its own residues and the carry of the steps before, a lane replays its 16
// positions sequentially, which yields its own first maximum; one butterfly picks the largest, the lower lane on ties.  The carry (prefix
// sum, running minimum and its position, best score with its start and end) is wave-uniform and goes to the next step.  The reverse strand
// is read backwards from the stored query and complemented through the 256-byte LDS table (nuclComplement, ref_rules.hpp), like the Hamming
// and the mode 3 kernels do.  Identities of the winning segment are counted in a second, byte-per-lane pass, only where the reference
// counts them.  Lane 0 writes the record and the keep flag; the kept records are compacted per query in input order (compactCsr).
// Overlaps of <= 64 residues take the same path (a lane-per-pair kernel for them has not been measured).
// Algorithmic bytes per candidate: 16 (candidate) + 16 (two packed offset / length words) + 2 * overlap per wrap tried + 2 * segment
// (identities) + 4 + 64 (flag, record) written, 64 per kept record copied once more; unmeasured, see DESIGN.md.
#include "common.hpp"
#include "../../include/plasship_ext/linclust.h"
#include "device_utils.hpp"
#include "host_util.hpp"
#include "ref_rules.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

namespace plasship {

struct LocalArgs {
    SeqView db;
    const CandHit *hits;
    uint64_t nHits;
    uint32_t *keep;              // [nHits] 1: the pair's record is written
    AlnRec *recs;                // [nHits] the record of pair h in slot h (valid where keep[h])
    const uint32_t *minScore;    // [minScoreLen] the smallest raw score that passes -e for that query length
    uint32_t minScoreLen;
    const signed char *mat;      // 123 x 123 in global memory, staged to LDS
    int reverseCapable;
    int covMode; float covThr;
    float seqIdThr; int alnLenThr, seqIdMode;
    int filterHits; float scorePerColThr;
    double lambda, logK, ln2;
    unsigned long long *stats;   // [0] records kept, [1] residues scored, [2] ids out of range
};

constexpr int LC_BLOCK = 256;
constexpr unsigned LC_PER_LANE = 16;
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
        unsigned char qa[LC_PER_LANE], tb[LC_PER_LANE];
        if (n == LC_PER_LANE) {
            uint32_t y[4]; __builtin_memcpy(y, t + to + i0, 16);
            uint32_t x[4];
            if (REV) {      // the 16 stored bytes that END at the mirrored position, last byte first
                uint32_t v[4]; __builtin_memcpy(v, q + (qLen - 1u - (qo + i0)) - 15u, 16);
                x[0] = __builtin_bswap32(v[3]); x[1] = __builtin_bswap32(v[2]); x[2] = __builtin_bswap32(v[1]); x[3] = __builtin_bswap32(v[0]);
            } else __builtin_memcpy(x, q + qo + i0, 16);
#pragma unroll
            for (unsigned j = 0; j < LC_PER_LANE; j++) { qa[j] = (unsigned char) (x[j >> 2] >> (8 * (j & 3))); tb[j] = (unsigned char) (y[j >> 2] >> (8 * (j & 3))); }
        } else {
#pragma unroll
            for (unsigned j = 0; j < LC_PER_LANE; j++) {
                const bool in = j < n;
                qa[j] = in ? (unsigned char) (REV ? q[qLen - 1u - (qo + i0 + j)] : q[qo + i0 + j]) : (unsigned char) 0;
                tb[j] = in ? (unsigned char) t[to + i0 + j] : (unsigned char) 0;
            }
        }
        int c[LC_PER_LANE];
#pragma unroll
        for (unsigned j = 0; j < LC_PER_LANE; j++) {
            const unsigned a = REV ? (unsigned) comp[qa[j]] : (unsigned) qa[j];
            c[j] = j < n ? (int) smat[((a & 127u) << 7) | (tb[j] & 127u)] : 0;
        }
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
    __shared__ signed char smat[128 * 128];              // row stride 128, rows and columns 123 .. 127 are 0: the index of a column is (a & 127) << 7 | (b & 127)
    __shared__ unsigned char sComp[256];
    for (int i = threadIdx.x; i < 128 * 128; i += LC_BLOCK) smat[i] = ((i & 127) < 123 && (i >> 7) < 123) ? a.mat[(i >> 7) * 123 + (i & 127)] : (signed char) 0;
    for (int i = threadIdx.x; i < 256; i += LC_BLOCK) sComp[i] = nuclComplement((unsigned char) i);
    __syncthreads();
    const unsigned lane = (unsigned) laneId();
    const uint64_t wavesPerBlock = LC_BLOCK / WAVE, stride = (uint64_t) gridDim.x * wavesPerBlock;
    unsigned long long nKept = 0, nScored = 0, nBad = 0;      // (wave-uniform; lane 0 adds them up at the end)
    for (uint64_t h = (uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE; h < a.nHits; h += stride) {
        const CandHit hit = a.hits[h];
        const uint32_t qid = hit.query, tid = hit.target;
        if (qid >= a.db.n || tid >= a.db.n) { nBad++; if (lane == 0) a.keep[h] = 0; continue; }
        const uint64_t qv = a.db.offLen[qid], tv = a.db.offLen[tid];
        const char *q = a.db.data + (qv >> 24), *t = a.db.data + (tv >> 24);
        const unsigned qLen = (unsigned) qv & 0xFFFFFFu, tLen = (unsigned) tv & 0xFFFFFFu;
        const bool isReverse = a.reverseCapable && hit.prefScore < 0;
        const bool isIdentity = qid == tid;                  // (one DB is query and target: sameQTDB)
        AlnRec rec; memset(&rec, 0, sizeof(rec));
        rec.query = qid; rec.target = tid;
        bool kept = false;
        if (canBeCovered(a.covThr, a.covMode, (float) qLen, (float) tLen)) {
            int bScore = 0, bStart = -1, bEnd = -1, bDiag = 0; unsigned bDiagLen = 0, bDist = 0;
            const unsigned d16 = hit.diag16 & 0xFFFFu;
            auto tryDiagonal = [&](int real, unsigned dist, unsigned qo, unsigned to, unsigned len) {
                const LocalBest s = isReverse ? scanDiagonal<true>(q, qLen, qo, t, to, len, smat, sComp, lane) : scanDiagonal<false>(q, qLen, qo, t, to, len, smat, sComp, lane);
                nScored += len;
                if (s.score > bScore) { bScore = s.score; bStart = s.start; bEnd = s.end; bDiag = real; bDiagLen = len; bDist = dist; }
            };
            // DistanceCalculator.h:98-111,119-173: a wrap that misses the sequences scores 0 and never wins
            for (unsigned d = 1; d <= 1u + tLen / 32768u; d++) {
                const unsigned dist = d * 65536u - d16;
                if (dist < tLen) tryDiagonal(-(int) dist, dist, 0u, dist, min(tLen - dist, qLen));
            }
            for (unsigned d = 0; d <= qLen / 65536u; d++) {
                const unsigned dist = d * 65536u + d16;
                if (dist < qLen) tryDiagonal((int) dist, dist, dist, 0u, min(tLen, qLen - dist));
            }
            // ---- wave-uniform finish (rescorediagonal.cpp:231-314) ----
            const int distance = bScore;
            const int bitScore = (int) (fma(a.lambda, (double) distance, -a.logK) / a.ln2 + 0.5);
            const int alnLen = (bEnd - bStart) + 1;
            int qS, qE, dS, dE;
            if (bDiag >= 0) { qS = bStart + (int) bDist; qE = bEnd + (int) bDist; dS = bStart; dE = bEnd; }
            else { qS = bStart; qE = bEnd; dS = bStart + (int) bDist; dE = bEnd + (int) bDist; }
            const uint32_t ms = (qLen < a.minScoreLen) ? a.minScore[qLen] : 0xFFFFFFFFu;
            const bool hasEvalue = (uint32_t) distance >= ms;
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
            const bool hasCov = hasCoverage(a.covThr, a.covMode, queryCov, targetCov);
            const bool hasSeqId = (double) seqId >= (double) (a.seqIdThr - FLT_EPSILON);
            const bool hasAlnLen = alnLen >= a.alnLenThr;
            const bool hasToFilter = a.filterHits && scorePerCol >= a.scorePerColThr;
            kept = isIdentity || hasToFilter || (hasAlnLen && hasCov && hasSeqId && hasEvalue);
            rec.bitScore = bitScore; rec.rawScore = distance; rec.seqId = seqId;
            rec.qStart = qS; rec.qEnd = qE; rec.qLen = (int) qLen; rec.dbStart = dS; rec.dbEnd = dE; rec.dbLen = (int) tLen;
            rec.alnLen = alnLen; rec.reversed = isReverse ? 1 : 0;
        }
        rec.accepted = kept ? 1 : 0; rec.btKind = 1;           // ungapped: the backtrace is one run of alnLen 'M'
        if (kept) nKept++;
        if (lane == 0) { a.keep[h] = kept ? 1u : 0u; a.recs[h] = rec; }
    }
    if (lane == 0) {
        if (nKept) atomicAdd(&a.stats[0], nKept);
        if (nScored) atomicAdd(&a.stats[1], nScored);
        if (nBad) atomicAdd(&a.stats[2], nBad);
    }
}

}  // namespace plasship
using namespace plasship;

// subset != nullptr: the E-value's database size is the residue count of the subset's representatives (plasship_rescore_local_subset)
static int rescoreLocal(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *subset, const plasship_local_params *par,
                        plasship_alns **out, plasship_rescore_stats *stats, const char *what) {
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
    DevBuf dKeep, dRecs, dStats, dMinScore, dMat;
    if (dKeep.alloc(std::max<uint64_t>(nHits, 1) * 4) != hipSuccess || dRecs.alloc(std::max<uint64_t>(nHits, 1) * sizeof(AlnRec)) != hipSuccess ||
        dStats.alloc(32) != hipSuccess || dMinScore.alloc((size_t) tabLen * 4) != hipSuccess || dMat.alloc(123 * 123) != hipSuccess) {
        setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 32, ctx->stream));
    { const int rc = stagedCopyToDevice(ctx, dMinScore.p, minScore.data(), (uint64_t) tabLen * 4); if (rc) return rc; }
    { const int rc = stagedCopyToDevice(ctx, dMat.p, asciiSubMat(nucl), 123 * 123); if (rc) return rc; }
    { const int rc = ensureOffLen(ctx, db); if (rc) return rc; }
    LocalArgs a; memset(&a, 0, sizeof(a));
    a.db = db->view(); a.hits = c->d_hits.as<CandHit>(); a.nHits = nHits; a.keep = dKeep.as<uint32_t>(); a.recs = dRecs.as<AlnRec>();
    a.minScore = dMinScore.as<uint32_t>(); a.minScoreLen = tabLen; a.mat = dMat.as<signed char>(); a.reverseCapable = c->reverseCapable;
    a.covMode = par->cov_mode; a.covThr = par->cov_thr; a.seqIdThr = par->seq_id_thr; a.alnLenThr = par->min_aln_len; a.seqIdMode = par->seq_id_mode;
    a.filterHits = !std::isnan(par->score_per_col_thr); a.scorePerColThr = a.filterHits ? par->score_per_col_thr : 0.0f;
    a.lambda = ev.g[0]; a.logK = ev.logK; a.ln2 = ev.ln2; a.stats = dStats.as<unsigned long long>();
    PH_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (nHits) {
        const unsigned grid = (unsigned) std::min<uint64_t>((nHits + LC_BLOCK / WAVE - 1) / (LC_BLOCK / WAVE), (uint64_t) ctx->numCU * 8);
        hipLaunchKernelGGL(rescoreLocalKernel, dim3(grid), dim3(LC_BLOCK), 0, ctx->stream, a);
    }
    PH_CHECK(hipEventRecord(ctx->ev[1], ctx->stream));
    unsigned long long hs[4] = {0, 0, 0, 0};
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hs[2]) { setError(std::string(what) + ": the candidate list names sequences that are not in the DB"); return PLASSHIP_ERR_ARG; }
    const uint64_t nKept = hs[0];
    std::unique_ptr<plasship_alns> holder(new plasship_alns());     // released to the caller on success only
    plasship_alns *al = holder.get();
    al->nQueries = nQ; al->nucl = nucl; al->addBacktrace = par->add_backtrace != 0; al->dbResidues = residues;
    al->nLines = nKept; al->nSlots = nKept; al->sparse = false; al->selfPending = false; al->qdb = db; al->tdb = db;
    // the kept records in input order, and the CSR over them
    if (const int rc = compactCsr(ctx, what, c->d_qoff.as<uint64_t>(), nQ, dRecs.p, sizeof(AlnRec), dKeep.as<uint32_t>(), nHits, nKept, al->d_qoff, al->d_recs)) return rc;
    if (stats) {
        stats->n_scored = nHits; stats->n_accepted = nKept; stats->overlap_residues = hs[1];
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); stats->ms_kernel = ms;
    }
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
