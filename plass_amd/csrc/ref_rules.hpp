// The reference's per-pair rules, once each: what byte parity of every module that gates, scores or complements a pair rests on.
// Device code; file:line in lib/mmseqs/src of the reference.  -ffp-contract=off: none of the float expressions below may be fused.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace plasship
