// The reference's per-alignment rules of the extension modules, once each: what byte parity of assembleresults, nuclassembleresults and
// guidedassembleresults rests on.  Product code (assemble.hip, rescore.hip); plain C++ as well, so that tests/test_host.py can compile it
// with g++ and check it against hand-made cases without a GPU.  file:line in src/assembler and lib/mmseqs/src/alignment of the reference.
// -ffp-contract=off: none of the float expressions below may be fused, and none may change its order or its types.
#pragma once
#include <cmath>
#include <cstdlib>
#if defined(__HIPCC__)
#define PLASSHIP_AR_HD __host__ __device__ __forceinline__
#else
#define PLASSHIP_AR_HD static inline __attribute__((always_inline))
#endif
namespace plasship {

struct AlnCoords { int qStart, qEnd, dbStart, dbEnd; };
struct DiagSpan { bool hit = false; unsigned qo = 0, to = 0, len = 0; };      // overlap of one diagonal: query offset, target offset, columns; hit = false: none

// Matcher::computeAlnLength on the starts parseAlignmentRecord adjusts, -1 -> 0 (Matcher.cpp:201-203,272-276)
PLASSHIP_AR_HD int alnLengthOf(int qStart, int qEnd, int dbStart, int dbEnd) {
    const int aq = (qStart == -1) ? 0 : qStart, ad = (dbStart == -1) ? 0 : dbStart;
    const int dq = abs(qEnd - aq), dd = abs(dbEnd - ad);
    return (dq > dd ? dq : dd) + 1;
}
// (int) (computeRawScoreFromBitScore(bits) + 0.5) (assembleresult.cpp:163, EvalueComputation.h:22-24; the reference binary fuses
// logK + bits * ln2)
PLASSHIP_AR_HD int rawScoreOfBits(int bitScore, double ln2, double logK, double lambda) {
    return (int) (fma((double) bitScore, ln2, logK) / lambda + 0.5);
}
// (int) (scorePerCol * 100): the queue's score, of a parsed hit's raw score (int, assembleresult.cpp:164,169) and of a re-scored hit's
// diagonal score (unsigned, assembleresult.cpp:100-101)
template <typename S> PLASSHIP_AR_HD int scorePerCol100(S score, unsigned alnLen) {
    const float scorePerCol = (float) score / (float) ((double) alnLen + 0.5);
    return (int) (scorePerCol * 100);
}
// ungappedAlignmentByDiagonal's overlap geometry (DistanceCalculator.h:119-125,148-150)
PLASSHIP_AR_HD DiagSpan diagonalSpan(int diag, unsigned qLen, unsigned tLen) {
    const unsigned dist = (unsigned) abs(diag);
    DiagSpan s;
    if (diag >= 0 && dist < qLen) { s.hit = true; s.qo = dist; s.len = tLen < qLen - dist ? tLen : qLen - dist; }
    else if (diag < 0 && dist < tLen) { s.hit = true; s.to = dist; s.len = tLen - dist < qLen ? tLen - dist : qLen; }
    return s;
}
// computeUngappedAlignment's walk over the wraps of a diagonal kept in 16 bits (DistanceCalculator.h:98-111): d16 - 65536 j for
// j = 1 .. 1 + tLen / 32768, then d16 + 65536 j for j = 0 .. qLen / 65536.  f(realDiagonal, span) for every wrap that meets the sequences,
// in that order; a wrap that misses them scores 0 there and never wins: f is not called for it.  The caller keeps the best, a strictly
// greater score replacing it.
template <typename F> PLASSHIP_AR_HD void forEachWrap(unsigned d16, unsigned qLen, unsigned tLen, F &&f) {
    for (unsigned j = 1; j <= 1u + tLen / 32768u; j++) {
        const int real = (int) (d16 - j * 65536u);
        const DiagSpan s = diagonalSpan(real, qLen, tLen);
        if (s.hit) f(real, s);
    }
    for (unsigned j = 0; j <= qLen / 65536u; j++) {
        const int real = (int) (j * 65536u + d16);
        const DiagSpan s = diagonalSpan(real, qLen, tLen);
        if (s.hit) f(real, s);
    }
}
// updateAlignment: the columns [startPos, endPos] of a diagonal as query and target coordinates (assembleresult.cpp:73-87)
PLASSHIP_AR_HD AlnCoords alnOnDiagonal(int diag, int startPos, int endPos) {
    const int dist = abs(diag);
    AlnCoords c;
    if (diag >= 0) { c.qStart = startPos + dist; c.qEnd = endPos + dist; c.dbStart = startPos; c.dbEnd = endPos; }
    else { c.qStart = startPos; c.qEnd = endPos; c.dbStart = startPos + dist; c.dbEnd = endPos + dist; }
    return c;
}
// updateAlignment's seqId (assembleresult.cpp:93).  A hit without a column has qStart == qEnd and no identity: 0 / 0 = NaN, which
// `seqId >= thr` drops (assembleresult.cpp:311)
PLASSHIP_AR_HD float rescoredSeqId(int ids, int qStart, int qEnd) {
    return (float) ids / ((float) qEnd - (float) qStart);
}
// selectFragmentToExtend without its identity test (assembleresult.cpp:47-52): a hit that starts at the target's first residue and leaves
// some of it over, or the same on the query, but not both
PLASSHIP_AR_HD bool isBranchType(int qStart, int qEnd, unsigned qLen, int dbStart, int dbEnd, unsigned dbLen) {
    const bool notBoth = !(dbStart == 0 && qStart == 0);
    const bool rightStart = dbStart == 0 && (dbEnd != (int) dbLen - 1);
    const bool leftStart = qStart == 0 && (qEnd != (int) qLen - 1);
    return (rightStart || leftStart) && notBoth;
}
// what a right extension would attach: the target's residues behind the alignment (assembleresult.cpp:212,234)
PLASSHIP_AR_HD unsigned rightFragLen(unsigned tLen, int dbEnd) { return tLen - ((unsigned) dbEnd + 1); }
// a hit of branch type with dbStart == 0 extends the untouched query to the right (assembleresult.cpp:212 at offset 0, :226) ...
PLASSHIP_AR_HD bool canExtendRight(unsigned fragR, int qEnd, unsigned qLen) { return fragR > 0 && (unsigned) qEnd == (qLen - 1); }
// ... one with qStart == 0 to the left (assembleresult.cpp:216 at offset 0, :250)
PLASSHIP_AR_HD bool canExtendLeft(int dbStart, int dbEnd, unsigned tLen) { return dbStart > 0 && (unsigned) dbEnd == (tLen - 1); }
// popped after the round's right extension of rightOff residues: deferred to the extended query if it still reaches beyond it
// (assembleresult.cpp:212,226-232), else dropped; qLen is the query's length before the round
PLASSHIP_AR_HD bool deferredRight(unsigned fragR, int qEnd, unsigned qLen, unsigned rightOff) {
    return fragR > rightOff && (unsigned) qEnd == (qLen - 1) && rightOff > 0;
}
// the same after the round's left extension of leftOff residues (assembleresult.cpp:216,250-256)
PLASSHIP_AR_HD bool deferredLeft(int dbStart, int dbEnd, unsigned tLen, unsigned leftOff) {
    return dbStart > (int) leftOff && (unsigned) dbEnd == (tLen - 1) && leftOff > 0;
}
// a reverse-strand hit (qStart > qEnd) put on the query's strand (nuclassembleresult.cpp:207-216)
PLASSHIP_AR_HD AlnCoords mirrorReverseHit(int qStart, int qEnd, int dbStart, int dbEnd, unsigned dbLen) {
    AlnCoords c;
    c.qStart = qEnd; c.qEnd = qStart;
    c.dbStart = (int) (dbLen - (unsigned) dbEnd - 1); c.dbEnd = (int) (dbLen - (unsigned) dbStart - 1);
    return c;
}

}  // namespace plasship
