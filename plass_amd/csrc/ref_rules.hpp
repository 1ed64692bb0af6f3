// The reference's per-pair rules, once each: what byte parity of every module that gates, scores or complements a pair rests on.
// Device code; file:line in lib/mmseqs/src of the reference.  -ffp-contract=off: none of the float expressions below may be fused.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include "common.hpp"

namespace plasship {

// Util::canBeCovered (commons/Util.cpp:533-550); COV_MODE_TARGET = 1, COV_MODE_QUERY = 2 (commons/Parameters.h:246-251)
__device__ __forceinline__ bool canBeCovered(float covThr, int covMode, float q, float t) {
    switch (covMode) {
        case 0: return (q / t >= covThr) && (t / q >= covThr);
        case 1: return (q / t) >= covThr;
        case 2: return (t / q) >= covThr;
        case 3: return ((t / q) >= covThr) && (t / q) <= 1.0f;
        case 4: return ((q / t) >= covThr) && (q / t) <= 1.0f;
        case 5: return (fminf(t, q) / fmaxf(t, q)) >= covThr;
        default: return true;
    }
}
// Util::hasCoverage (commons/Util.cpp:552-568)
__device__ __forceinline__ bool hasCoverage(float covThr, int covMode, float qc, float tc) {
    switch (covMode) {
        case 0: return (qc >= covThr) && (tc >= covThr);
        case 1: return tc >= covThr;
        case 2: return qc >= covThr;
        default: return true;
    }
}
// SmithWaterman::computeCov (alignment/StripedSmithWaterman.cpp:1055-1057)
__device__ __forceinline__ float computeCov(unsigned s, unsigned e, unsigned len) {
    return (float) (min(len, max(s, e)) - min(s, e) + 1) / (float) len;
}
// Util::computeSeqId (commons/Util.cpp:588-598): SEQ_ID_ALN_LEN = 0, SEQ_ID_SHORT = 1, SEQ_ID_LONG = 2; every argument an int, as there
// (0 / 0 = NaN where the caller has no aligned column: the Hamming rescore relies on it)
__device__ __forceinline__ float computeSeqId(int seqIdMode, int ids, int qLen, int tLen, int alnLen) {
    switch (seqIdMode) {
        case 0: return (float) ids / (float) alnLen;
        case 1: return (float) ids / (float) min(qLen, tLen);
        case 2: return (float) ids / (float) max(qLen, tLen);
        default: return 0.0f;
    }
}
// num2aa[reverseResidue(aa2num[c])], the letter of the other strand (alignment/rescorediagonal.cpp:175-178 with the letter mapping of
// commons/NucleotideMatrix.cpp:17-61): the case and the IUPAC codes fold onto A, C, G, T, everything else onto X; always upper case
__device__ __forceinline__ unsigned char nuclComplement(unsigned char c) {
    switch (c & ~0x20) {
        case 'A': return 'T';
        case 'C': case 'M': case 'Y': case 'H': return 'G';
        case 'T': case 'U': case 'W': return 'A';
        case 'G': case 'K': case 'B': case 'D': case 'V': case 'R': case 'S': return 'C';
        default: return 'X';
    }
}

// ---- rescorediagonal's pair rules (alignment/rescorediagonal.cpp), shared by the list-in, list-out rescore kernels of modes 0, 1 and 2 ----
// One candidate pair as a kernel meets it: the two entries from their packed offset / length words (ensureOffLen), and the strand the
// query is read on (rescorediagonal.cpp:170-181: a negative prefilter score in a list with strands).  bad: an id that is not in its DB;
// nothing else is set then.  One DB is query and target where t is left out.
struct PairSeqs { const char *q, *t; unsigned qLen, tLen; bool rev, bad; };
__device__ __forceinline__ PairSeqs loadPair(const CandHit &hit, int reverseCapable, const SeqView &q, const SeqView &t) {
    PairSeqs p; p.q = nullptr; p.t = nullptr; p.qLen = 0; p.tLen = 0; p.rev = false;
    p.bad = hit.query >= q.n || hit.target >= t.n;
    if (p.bad) return p;
    const uint64_t qv = q.offLen[hit.query], tv = t.offLen[hit.target];
    p.q = q.data + (qv >> 24); p.t = t.data + (tv >> 24);
    p.qLen = (unsigned) qv & 0xFFFFFFu; p.tLen = (unsigned) tv & 0xFFFFFFu;
    p.rev = reverseCapable && hit.prefScore < 0;
    return p;
}
__device__ __forceinline__ PairSeqs loadPair(const CandHit &hit, int reverseCapable, const SeqView &db) { return loadPair(hit, reverseCapable, db, db); }
// EvalueComputation::computeBitScore, truncated as rescorediagonal.cpp:241 does (the reference binary fuses lambda * score - logK)
__device__ __forceinline__ int bitScoreOf(int rawScore, double lambda, double logK, double ln2) {
    return (int) (fma(lambda, (double) rawScore, -logK) / ln2 + 0.5);
}
// evalue <= evalThr (rescorediagonal.cpp:243,306) as a comparison with the smallest raw score that passes for the query's length
// (evalueGateTable, common.hpp); a length the table does not hold passes nothing
__device__ __forceinline__ bool passesEvalue(int rawScore, unsigned qLen, const uint32_t *__restrict__ minScore, uint32_t minScoreLen) {
    const uint32_t ms = (qLen < minScoreLen) ? minScore[qLen] : 0xFFFFFFFFu;
    return (uint32_t) rawScore >= ms;
}
// The thresholds of the accept rule, and the rule (rescorediagonal.cpp:304-332); filterHits = 0 where the mode has no --filter-hits
struct AcceptThr { int covMode; float covThr, seqIdThr; int alnLenThr, filterHits; float scorePerColThr; };
__device__ __forceinline__ bool acceptsPair(const AcceptThr &p, bool isIdentity, bool hasEvalue, float seqId, int alnLen, float queryCov, float targetCov, float scorePerCol) {
    const bool hasCov = hasCoverage(p.covThr, p.covMode, queryCov, targetCov);
    const bool hasSeqId = (double) seqId >= (double) (p.seqIdThr - FLT_EPSILON);
    const bool hasAlnLen = alnLen >= p.alnLenThr;
    const bool hasToFilter = p.filterHits && scorePerCol >= p.scorePerColThr;      // (a NaN, 0 / 0 where nothing scored, is never >= the threshold)
    return isIdentity || hasToFilter || (hasAlnLen && hasCov && hasSeqId && hasEvalue);
}
// the line of a sequence with itself as kmermatcher adds it to every entry, score 0 on diagonal 0: the implicit self line
// (plasship_cands::nNonSelf counts the kept lines that are not of this kind)
__device__ __forceinline__ bool isImplicitSelfLine(bool isIdentity, int32_t prefScore, unsigned diag16) { return isIdentity && prefScore == 0 && diag16 == 0; }

}  // namespace plasship
