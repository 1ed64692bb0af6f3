// plasship: mergereads — paired-end FASTQ -> read DB (replaces int mergereads(int, const char**, const Command&),
// src/assembler/mergereads.cpp:15-129, which runs FLASH's combine_reads per pair, lib/flash/combine_reads.cpp).  Product code.
//
//   host    the FASTQ files are read (plain: pread on the host threads; .gz: one zlib stream per mate, the two mates on two threads,
//           zlib dlopen'ed as libz.so.1), validated and indexed on the host threads, then packed batch by batch (pairs with both mates'
//           sequence and quality, 4-byte aligned) and uploaded through the context's pinned double buffer; packing batch b+1 overlaps
//           the kernels of batch b (they run on the stream while the host packs)
//   device  mergePairsKernel (both mates <= 512 bases: one 16-lane row per pair, mates staged in LDS, four bases per dword) and
//           mergePairsWaveKernel (longer mates: one wave per pair) decide every pair; the entry and byte counts are scanned (scan.hip)
//           and mergeWriteKernel writes the merged read, or mate 1 and the reverse complement of mate 2, straight into the resident
//           read DB ("SEQ\n\0", keys 0..n-1 in input order)
//   headers the kseq names stay on the host and become the header DB (dbtype 12, "name\n\0") once the decisions are downloaded.
#include "common.hpp"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

namespace plasship {

// ---- semantics (mergereads.cpp:19-23, combine_reads.cpp:266-470, read.cpp) --------------------------------------------------------
// reverse_complement (lib/flash/read.cpp:3-8): IUPAC codes and their lowercase forms complemented, U -> A, every other byte '.'
struct CompTable { unsigned char c[256]; };
static CompTable makeCompTable() {
    CompTable t; memset(t.c, '.', 256);
    const char *from = "ACGTUNSWRYKMBDHV", *to = "TGCAANSWYRMKVHDB";
    for (int k = 0; from[k]; k++) { t.c[(unsigned char) from[k]] = (unsigned char) to[k]; t.c[(unsigned char) from[k] + 32] = (unsigned char) to[k] + 32; }
    return t;
}

// one pair of a batch: its packed record at `off` (4-byte aligned): mate 1 sequence, mate 1 quality, mate 2 sequence, mate 2 quality
// (as read, NOT reverse-complemented), each padded with zero bytes to a multiple of 4
struct PairMeta { uint64_t off; uint32_t l1, l2; };
__host__ __device__ inline uint64_t pad4(uint64_t x) { return (x + 3) & ~3ull; }

constexpr int MR_MAX_SMALL = 512;                      // mates the row kernel takes (Illumina reads are <= 300)
constexpr int MR_WORDS = MR_MAX_SMALL / 4 + 2;         // + the word a shifted read of the last word touches
constexpr int MR_ROWS = 16;                            // pairs per 256-thread workgroup
constexpr int MIN_OVERLAP = 15, MAX_OVERLAP = 65;      // mergereads.cpp:19-20
#define MR_MAX_DENSITY 0.10f                            // mergereads.cpp:21 (max_mismatch_density is a float)

// high bit of every byte of x that is not zero (exact: no carry leaves a byte)
__device__ __forceinline__ uint32_t byteNonZero(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
__device__ __forceinline__ uint32_t highToBytes(uint32_t hi) { return (hi >> 7) * 0xFFu; }

// one overlap word: four positions of the overlap of read 1 (a, qa) with read 2 (b, qb); vm = high bits of the positions inside it.
// compute_mismatch_stats (combine_reads.cpp:73-249): a position where either base is 'N' is uncalled (only reads that hold an 'N' have
// such positions, so testing always is the same as testing under haveN); otherwise a differing base counts as a mismatch and adds the
// smaller of the two quality bytes.  Quality bytes are < 128 (refused otherwise), where the SSE2 path's unsigned minimum and the scalar
// path's signed one agree; then (qa | 0x80) - qb per byte never borrows and its high bit says qa >= qb.
__device__ __forceinline__ void overlapWord(uint32_t a, uint32_t b, uint32_t qa, uint32_t qb, uint32_t vm, uint32_t &mism, uint32_t &unc, uint32_t &qsum) {
    const uint32_t bm = highToBytes(vm);
    qa &= bm; qb &= bm;
    const uint32_t un = ((~byteNonZero(a ^ 0x4E4E4E4Eu)) | (~byteNonZero(b ^ 0x4E4E4E4Eu))) & vm;
    const uint32_t mm = byteNonZero(a ^ b) & vm & ~un;
    const uint32_t geMask = highToBytes(((qa | 0x80808080u) - qb) & 0x80808080u);       // bytes where qa >= qb
    const uint32_t qmin = (qb & geMask) | (qa & ~geMask);
    mism += __popc(mm); unc += __popc(un);
    qsum = __builtin_amdgcn_sad_u8(qmin & highToBytes(mm), 0u, qsum);
}

// pair_align's candidate test and key for one offset: overlap >= 15 after the uncalled positions, score_len = min(len, 65) as a float,
// both ratios IEEE float divisions of the unsigned counts (the compiler's default, correctly rounded f32 divide).  The sequential update
// rule (:304-313: take the candidate if density < best, or density == best and qual < best) starting from density 1.1f keeps the FIRST
// offset with the lexicographically smallest (density, qual) — no density reaches 1.1f exactly — so the key (density, qual) as the two
// float bit patterns (non-negative floats order like their bits), ties broken by the smaller offset, is a valid parallel reduction.
__device__ __forceinline__ unsigned long long candKey(int len, uint32_t mism, uint32_t qsum) {
    if (len < MIN_OVERLAP) return ~0ull;
    const float sl = (float) min(len, MAX_OVERLAP);
    const float q = (float) qsum / sl, d = (float) mism / sl;
    return ((unsigned long long) __float_as_uint(d) << 32) | __float_as_uint(q);
}

__device__ __forceinline__ unsigned long long rowMin16U64(unsigned long long v) {
    unsigned long long o;
    o = dppMov64<0xB1>(v); v = o < v ? o : v;
    o = dppMov64<0x4E>(v); v = o < v ? o : v;
    o = dppMov64<0x141>(v); v = o < v ? o : v;
    o = dppMov64<0x140>(v); v = o < v ? o : v;
    return v;
}

struct MergeArgs {
    const char *pk; const PairMeta *meta; uint32_t n;      // the batch
    const unsigned char *comp;                             // CompTable (device)
    const uint32_t *bigList; uint32_t nBig;                // pairs with a mate > 512 bases (wave kernel)
    uint8_t *status;                                       // [n] 1 combined, 0 not
    int32_t *pos;                                          // [n] overlap begin of a combined pair
    uint32_t *nEnt; uint64_t *nBytes;                      // [n] entries / entry bytes the pair writes
};

__device__ __forceinline__ void pairResult(const MergeArgs &a, uint32_t p, uint32_t l1, uint32_t l2, unsigned long long key, uint32_t best) {
    const bool comb = key != ~0ull && __uint_as_float((uint32_t) (key >> 32)) <= MR_MAX_DENSITY;    // :330 best_mismatch_density > max -> NO_ALIGNMENT
    a.status[p] = comb ? 1 : 0;
    a.pos[p] = comb ? (int32_t) best : -1;
    a.nEnt[p] = comb ? 1u : 2u;
    // combined length = L1 + L2 - overlap = L2 + pos (generate_combined_read, :346-351)
    a.nBytes[p] = comb ? (uint64_t) l2 + best + 2 : (uint64_t) l1 + l2 + 4;
}

// one 16-lane row per pair (four pairs per wave), both mates <= 512 bases.  The row stages the two sequences and quality strings in LDS
// (mate 2 reverse-complemented on the way in, mergereads.cpp:77), then every lane takes the offsets start + lane, + 16, ... and compares
// four positions per dword: read 1 at an arbitrary byte offset is two aligned LDS words funnel-shifted (v_alignbyte), read 2 starts at 0.
__global__ __launch_bounds__(256) void mergePairsKernel(MergeArgs a) {
    __shared__ uint32_t sh[MR_ROWS][4][MR_WORDS];
    __shared__ unsigned char comp[256];
    const int r = threadIdx.x >> 4, l = threadIdx.x & 15;
    comp[threadIdx.x] = a.comp[threadIdx.x];
    for (uint64_t b0 = (uint64_t) blockIdx.x * MR_ROWS; b0 < a.n; b0 += (uint64_t) gridDim.x * MR_ROWS) {     // uniform trip count: barriers below
        const uint64_t p = b0 + r;
        uint32_t l1 = 0, l2 = 0;
        bool act = false;
        uint32_t *S1 = sh[r][0], *Q1 = sh[r][1], *S2 = sh[r][2], *Q2 = sh[r][3];
        __syncthreads();                                    // comp filled / the previous pair's words read
        if (p < a.n) {
            const PairMeta m = a.meta[p];
            l1 = m.l1; l2 = m.l2;
            act = l1 <= MR_MAX_SMALL && l2 <= MR_MAX_SMALL;
            if (act) {
                const uint32_t *g = reinterpret_cast<const uint32_t *>(a.pk + m.off);
                const uint32_t w1 = (l1 + 3) >> 2, w2 = (l2 + 3) >> 2;
                for (uint32_t w = l; w < w1; w += 16) { S1[w] = g[w]; Q1[w] = g[w1 + w]; }
                if (l == 0) { S1[w1] = 0; Q1[w1] = 0; S1[w1 + 1] = 0; Q1[w1 + 1] = 0; }
                unsigned char *S2b = reinterpret_cast<unsigned char *>(S2), *Q2b = reinterpret_cast<unsigned char *>(Q2);
                for (uint32_t w = l; w < w2; w += 16) {
                    const uint32_t s = g[2 * w1 + w], q = g[2 * w1 + w2 + w];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t t = 4 * w + k;
                        if (t < l2) { S2b[l2 - 1 - t] = comp[(s >> (8 * k)) & 0xFFu]; Q2b[l2 - 1 - t] = (unsigned char) (q >> (8 * k)); }
                    }
                }
            }
        }
        __syncthreads();
        unsigned long long best = ~0ull; uint32_t bestPos = 0x7FFFFFFFu;
        if (act) {
            const int start = max(0, (int) l1 - (int) l2), last = (int) l1 - MIN_OVERLAP;   // :287-289
            for (int i = start + l; i <= last; i += 16) {
                const int ov = (int) l1 - i, nw = (ov + 3) >> 2, sft = i & 3, base = i >> 2;
                uint32_t mism = 0, unc = 0, qsum = 0;
                for (int k = 0; k < nw; k++) {
                    const uint32_t s1 = __builtin_amdgcn_alignbyte(S1[base + k + 1], S1[base + k], sft);
                    const uint32_t q1 = __builtin_amdgcn_alignbyte(Q1[base + k + 1], Q1[base + k], sft);
                    const int rem = ov - 4 * k;
                    const uint32_t vm = rem >= 4 ? 0x80808080u : (0x80808080u & ((1u << (8 * rem)) - 1u));
                    overlapWord(s1, S2[k], q1, Q2[k], vm, mism, unc, qsum);
                }
                const unsigned long long key = candKey(ov - (int) unc, mism, qsum);
                if (key < best) { best = key; bestPos = (uint32_t) i; }           // offsets rise per lane: ties keep the first
            }
        }
        const unsigned long long kmin = rowMin16U64(best);
        const uint32_t pmin = rowMin16U32(best == kmin ? bestPos : 0x7FFFFFFFu);
        if (act && l == 0) pairResult(a, (uint32_t) p, l1, l2, kmin, pmin);
    }
}

// one wave per pair with a mate longer than 512 bases (no length limit below int32): lanes take offsets, positions are read straight
// from the packed record, mate 2 reverse-complemented on the fly
__global__ __launch_bounds__(256) void mergePairsWaveKernel(MergeArgs a) {
    const int lane = laneId();
    for (uint64_t wv = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < a.nBig; wv += ((uint64_t) gridDim.x * blockDim.x) >> 6) {
        const uint32_t p = a.bigList[wv];
        const PairMeta m = a.meta[p];
        const int l1 = (int) m.l1, l2 = (int) m.l2;
        const unsigned char *s1 = reinterpret_cast<const unsigned char *>(a.pk + m.off), *q1 = s1 + pad4(m.l1);
        const unsigned char *s2 = q1 + pad4(m.l1), *q2 = s2 + pad4(m.l2);
        unsigned long long best = ~0ull; uint32_t bestPos = 0x7FFFFFFFu;
        const int start = max(0, l1 - l2), last = l1 - MIN_OVERLAP;
        for (int i = start + lane; i <= last; i += WAVE) {
            const int ov = l1 - i;
            uint32_t mism = 0, unc = 0, qsum = 0;
            for (int j = 0; j < ov; j++) {
                const unsigned char x = s1[i + j], y = a.comp[s2[l2 - 1 - j]];
                if (x == 'N' || y == 'N') { unc++; continue; }
                if (x != y) { mism++; qsum += min(q1[i + j], q2[l2 - 1 - j]); }
            }
            const unsigned long long key = candKey(ov - (int) unc, mism, qsum);
            if (key < best) { best = key; bestPos = (uint32_t) i; }
        }
        const unsigned long long own = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(best, o, 64); best = t < best ? t : best; }
        uint32_t pm = own == best ? bestPos : 0x7FFFFFFFu;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(pm, o, 64); pm = t < pm ? t : pm; }
        if (lane == 0) pairResult(a, p, (uint32_t) l1, (uint32_t) l2, best, pm);
    }
}

struct WriteArgs {
    const char *pk; const PairMeta *meta; uint32_t n;
    const unsigned char *comp;
    const uint8_t *status; const int32_t *pos;
    const uint64_t *entBase, *byteBase;                    // [n + 1] exclusive scans of nEnt / nBytes (scan.hip)
    const uint64_t *run;                                   // [2] entries / bytes the earlier batches wrote
    char *data; uint64_t *off; uint32_t *len; uint32_t *key; uint32_t *maxLen;
};

// writes every pair's entries into the resident DB: a combined pair as generate_combined_read builds it (combine_reads.cpp:389-465:
// read 1 before the overlap; in the overlap the agreeing base, else the base with the higher quality, on equal quality mate 2's unless
// it is 'N'; the rest of read 2), an uncombined pair as mate 1 and the reverse-complemented mate 2 (mergereads.cpp:96-115).  One row of
// 16 lanes per pair; the wave's rows move together so that the longest entry is reduced per wave before one atomic.
__global__ __launch_bounds__(256) void mergeWriteKernel(WriteArgs a) {
    const int l = threadIdx.x & 15, r = (threadIdx.x >> 4) & 3;
    const uint64_t wave0 = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6, nWaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    for (uint64_t wb = wave0 * 4; wb < a.n; wb += nWaves * 4) {
        const uint64_t p = wb + r;
        uint32_t longest = 0;
        if (p < a.n) {
            const PairMeta m = a.meta[p];
            const uint32_t l1 = m.l1, l2 = m.l2;
            const unsigned char *s1 = reinterpret_cast<const unsigned char *>(a.pk + m.off), *q1 = s1 + pad4(l1);
            const unsigned char *s2 = q1 + pad4(l1), *q2 = s2 + pad4(l2);
            const uint64_t e = a.run[0] + a.entBase[p], b = a.run[1] + a.byteBase[p];
            char *o = a.data + b;
            if (a.status[p]) {
                const uint32_t ps = (uint32_t) a.pos[p], outLen = l2 + ps;
                for (uint32_t k = l; k < outLen; k += 16) {
                    unsigned char c;
                    if (k < ps) c = s1[k];
                    else {
                        const uint32_t j = k - ps;
                        const unsigned char y = a.comp[s2[l2 - 1 - j]];
                        if (k < l1) {
                            const unsigned char x = s1[k], qx = q1[k], qy = q2[l2 - 1 - j];
                            c = x == y ? x : qx > qy ? x : qx < qy ? y : (y == 'N' ? x : y);
                        } else c = y;
                    }
                    o[k] = (char) c;
                }
                if (l == 0) { o[outLen] = '\n'; o[outLen + 1] = 0; a.off[e] = b; a.len[e] = outLen; a.key[e] = (uint32_t) e; }
                longest = outLen;
            } else {
                char *o2 = o + l1 + 2;
                for (uint32_t k = l; k < l1; k += 16) o[k] = (char) s1[k];
                for (uint32_t k = l; k < l2; k += 16) o2[k] = (char) a.comp[s2[l2 - 1 - k]];
                if (l == 0) {
                    o[l1] = '\n'; o[l1 + 1] = 0; o2[l2] = '\n'; o2[l2 + 1] = 0;
                    a.off[e] = b; a.len[e] = l1; a.key[e] = (uint32_t) e;
                    a.off[e + 1] = b + l1 + 2; a.len[e + 1] = l2; a.key[e + 1] = (uint32_t) (e + 1);
                }
                longest = max(l1, l2);
            }
        }
        const uint32_t w = (uint32_t) waveReduceMax((int) longest);     // mates are shorter than 2^31
        if (laneId() == 0 && w) atomicMax(a.maxLen, w);
    }
}

// the running totals the next batch's entries and bytes start at
__global__ void mergeRunKernel(uint64_t *run, const uint64_t *entBase, const uint64_t *byteBase, uint32_t n) {
    if (threadIdx.x == 0) { run[0] += entBase[n]; run[1] += byteBase[n]; }
}

// ---- host: FASTQ input (kseq semantics, lib/mmseqs/lib/ksw2/kseq.h; KSeqWrapper.cpp:160-195) -------------------------------------
// one record of a FASTQ file: offsets into the file's bytes
struct FastqRec { uint64_t name, seq, qual; uint32_t nameLen, len; };
struct FastqFile { std::string path; HostBytes buf; std::vector<FastqRec> rec; int rc = 0; std::string err; };

// the whole file into memory (host_util.cpp, readSeqFileBytes: shared with createdb.hip)
static int readFastqBytes(FastqFile &f) { return readSeqFileBytes(f.path, f.buf, f.err) ? PLASSHIP_OK : PLASSHIP_ERR_IO; }

static inline bool kseqSpace(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// Four-line FASTQ records, exactly what kseq_read (kseq.h:193-243) returns for them: the name up to the first isspace() byte, one sequence
// line, a '+' line, one quality line of the sequence's length; a '\r' before a line's '\n' is dropped when the line holds more than it
// (kseq.h:145).  Everything else is refused with PLASSHIP_ERR_UNSUPPORTED (then the reference reads the file): FASTA, multi-line records,
// blank lines, a truncated file, an empty sequence, a sequence line starting with '>', '@' or '+', a quality byte >= 128 (where FLASH's
// SSE2 and scalar paths disagree), a NUL byte in a sequence.  Records are found on all host threads: every record is four lines, so record
// r starts after newline 4r - 1.
static int parseFastq(FastqFile &f) {
    const char *B = f.buf.p; const uint64_t S = f.buf.n;
    f.rec.clear();
    if (S == 0) return PLASSHIP_OK;
    if (B[0] != '@') { f.err = f.path + ": not a FASTQ file (FASTA input is read by the reference)"; return PLASSHIP_ERR_UNSUPPORTED; }
    const int T = std::max(1, std::min<int>(hostThreads(), (int) (S >> 20) + 1));
    std::vector<uint64_t> cnt(T + 1, 0);
    auto chunk = [&](int c) { return S * (uint64_t) c / (uint64_t) T; };
    std::vector<std::thread> th;
    for (int c = 0; c < T; c++) th.emplace_back([&, c]() {
        uint64_t n = 0; const char *p = B + chunk(c), *e = B + chunk(c + 1);
        while (p < e && (p = (const char *) memchr(p, '\n', (size_t) (e - p)))) { n++; p++; }
        cnt[c + 1] = n;
    });
    for (auto &t : th) t.join();
    th.clear();
    for (int c = 0; c < T; c++) cnt[c + 1] += cnt[c];
    const uint64_t nLines = cnt[T] + (B[S - 1] != '\n' ? 1 : 0);
    if (nLines % 4) { f.err = f.path + ": not four-line FASTQ (multi-line records, blank lines or a truncated file are read by the reference)"; return PLASSHIP_ERR_UNSUPPORTED; }
    const uint64_t nRec = nLines / 4;
    if (nRec >= 0xFFFFFFFFull) { f.err = f.path + ": too many records"; return PLASSHIP_ERR_UNSUPPORTED; }
    std::vector<uint64_t> start(nRec + 1, 0);
    start[nRec] = S;
    for (int c = 0; c < T; c++) th.emplace_back([&, c]() {
        uint64_t g = cnt[c]; const char *p = B + chunk(c), *e = B + chunk(c + 1);
        while (p < e && (p = (const char *) memchr(p, '\n', (size_t) (e - p)))) {
            g++;                                                  // the line after this newline
            const uint64_t x = (uint64_t) (p - B) + 1;
            if ((g & 3) == 0 && x < S) start[g >> 2] = x;
            p++;
        }
    });
    for (auto &t : th) t.join();
    f.rec.resize(nRec);
    std::mutex mu; uint64_t firstBad = ~0ull; std::string badMsg;
    parallelRanges((size_t) nRec, [&](int, size_t rb, size_t re) {
        for (size_t r = rb; r < re; r++) {
            const uint64_t s = start[r], e = start[r + 1];
            const char *why = nullptr;
            auto eol = [&](uint64_t from) -> uint64_t { const void *q = memchr(B + from, '\n', (size_t) (e - from)); return q ? (uint64_t) ((const char *) q - B) : e; };
            const uint64_t e0 = eol(s), e1 = eol(e0 + 1), e2 = eol(e1 + 1), e3 = e2 + 1 <= e ? eol(e2 + 1) : e;
            FastqRec &R = f.rec[r];
            uint64_t nm = s + 1; while (nm < e0 && !kseqSpace((unsigned char) B[nm])) nm++;
            R.name = s + 1; R.nameLen = (uint32_t) (nm - s - 1);
            uint64_t sl = e1 - e0 - 1, ql = e3 - e2 - 1;
            if (sl > 1 && B[e1 - 1] == '\r') sl--;
            if (ql > 1 && B[e3 - 1] == '\r') ql--;
            R.seq = e0 + 1; R.qual = e2 + 1; R.len = (uint32_t) sl;
            const unsigned char *sq = reinterpret_cast<const unsigned char *>(B + R.seq), *qq = reinterpret_cast<const unsigned char *>(B + R.qual);
            if (B[s] != '@') why = "a record does not start with '@'";
            else if (B[e1 + 1] != '+') why = "multi-line sequence or a missing '+' line";
            else if (sl == 0) why = "an empty sequence";
            else if (sq[0] == '>' || sq[0] == '@' || sq[0] == '+') why = "a sequence line starting with '>', '@' or '+'";
            else if (ql != sl) why = "a quality string whose length differs from the sequence's (multi-line or truncated record)";
            else if (sl >= 0x7FFFFFF0ull) why = "a sequence of 2^31 bases or more";
            else {
                unsigned char orq = 0; bool nul = false;
                for (uint64_t k = 0; k < sl; k++) { orq |= qq[k]; nul |= sq[k] == 0; }
                if (orq & 0x80) why = "a quality byte >= 128";
                else if (nul) why = "a NUL byte in a sequence";
            }
            if (why) {
                std::lock_guard<std::mutex> g(mu);
                if (r < firstBad) { firstBad = r; badMsg = f.path + ": record " + std::to_string(r + 1) + ": " + why + " (read by the reference)"; }
            }
        }
    });
    if (firstBad != ~0ull) { f.err = badMsg; return PLASSHIP_ERR_UNSUPPORTED; }
    return PLASSHIP_OK;
}

static double msSince(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_mergereads(plasship_ctx *ctx, const char *const *fastq, size_t n_files, const plasship_merge_params *par,
                                   plasship_seqdb **reads, plasship_seqdb **headers, plasship_merge_stats *stats) {
    if (!ctx || !fastq || !reads || !headers || n_files < 2 || (n_files & 1)) { setError("plasship_mergereads: bad argument (an even number of FASTQ files, at least two)"); return PLASSHIP_ERR_ARG; }
    for (size_t k = 0; k < n_files; k++) if (!fastq[k]) { setError("plasship_mergereads: NULL file name"); return PLASSHIP_ERR_ARG; }
    if (par && (par->min_overlap != 15 || par->max_overlap != 65 || par->max_mismatch_density != 0.10f || par->allow_outies)) {
        setError("plasship_mergereads: only the parameters of the reference's mergereads are implemented (min_overlap 15, max_overlap 65, max_mismatch_density 0.10, no outies)");
        return PLASSHIP_ERR_UNSUPPORTED;
    }
    // KSeqFactory (KSeqWrapper.cpp:160-195): "stdin" and .bz2 are left to the reference
    for (size_t k = 0; k < n_files; k++) {
        const std::string p = fastq[k];
        if (p == "stdin") { setError("plasship_mergereads: reading stdin is left to the reference"); return PLASSHIP_ERR_UNSUPPORTED; }
        if (pathEndsWith(p, ".bz2")) { setError("plasship_mergereads: " + p + ": bzip2 input is left to the reference"); return PLASSHIP_ERR_UNSUPPORTED; }
    }
    PH_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const auto tParse0 = std::chrono::steady_clock::now();
    // ---- every file read and validated first: a refusal comes before anything is computed ----
    const size_t nFP = n_files / 2;
    std::vector<std::unique_ptr<FastqFile>> files(n_files);
    for (size_t k = 0; k < n_files; k++) { files[k].reset(new FastqFile()); files[k]->path = fastq[k]; }
    std::vector<uint64_t> pairBase(nFP + 1, 0);
    for (size_t fp = 0; fp < nFP; fp++) {
        FastqFile &A = *files[2 * fp], &B = *files[2 * fp + 1];
        std::thread tb([&]() { B.rc = readFastqBytes(B); });           // the two mates' streams on two threads
        A.rc = readFastqBytes(A);
        tb.join();
        for (FastqFile *f : {&A, &B}) if (f->rc) { setError("plasship_mergereads: " + f->err); return f->rc; }
        for (FastqFile *f : {&A, &B}) { f->rc = parseFastq(*f); if (f->rc) { setError("plasship_mergereads: " + f->err); return f->rc; } }
        pairBase[fp + 1] = pairBase[fp] + std::min(A.rec.size(), B.rec.size());       // mergereads.cpp:52: the shorter file ends the pair
    }
    const uint64_t N = pairBase[nFP];
    if (2 * N >= 0xFFFFFFFFull) { setError("plasship_mergereads: too many read pairs"); return PLASSHIP_ERR_UNSUPPORTED; }
    auto recOf = [&](uint64_t p, int mate) -> std::pair<const FastqFile *, const FastqRec *> {
        const size_t fp = (size_t) (std::upper_bound(pairBase.begin(), pairBase.end(), p) - pairBase.begin()) - 1;
        const FastqFile *f = files[2 * fp + mate].get();
        return {f, &f->rec[p - pairBase[fp]]};
    };
    // upper bound of the read DB: every pair unmerged
    uint64_t capBytes = 0;
    for (size_t fp = 0; fp < nFP; fp++)
        for (uint64_t i = 0; i < pairBase[fp + 1] - pairBase[fp]; i++) capBytes += (uint64_t) files[2 * fp]->rec[i].len + files[2 * fp + 1]->rec[i].len + 4;
    double msParse = msSince(tParse0), msUpload = 0, msKernel = 0;

    uint64_t batch = 4ull << 20;
    if (const char *e = getenv("PLASSHIP_MERGE_BATCH")) { const long long v = atoll(e); if (v > 0) batch = (uint64_t) v; }
    batch = std::max<uint64_t>(1, std::min<uint64_t>(batch, std::max<uint64_t>(N, 1)));

    std::unique_ptr<plasship_seqdb> o(new plasship_seqdb());
    DevBuf dComp, dStatus, dRun, dPk, dPos, dEnt, dBytes, dEntBase, dByteBase, dTmp;
    const size_t tmpBytes = exclusiveScanTmpBytes((size_t) batch + 1);
    if (o->d_data.allocLong(capBytes + 64) != hipSuccess || o->d_off.allocLong((2 * N + 1) * 8) != hipSuccess || o->d_len.allocLong((2 * N + 1) * 4) != hipSuccess ||
        o->d_key.allocLong((2 * N + 1) * 4) != hipSuccess || dComp.alloc(256) != hipSuccess || dStatus.alloc(N + 1) != hipSuccess || dRun.alloc(24) != hipSuccess ||
        dPos.alloc(batch * 4) != hipSuccess || dEnt.alloc((batch + 1) * 4) != hipSuccess || dBytes.alloc((batch + 1) * 8) != hipSuccess ||
        dEntBase.alloc((batch + 2) * 8) != hipSuccess || dByteBase.alloc((batch + 2) * 8) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess) {
        setError("plasship_mergereads: out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    static const CompTable comp = makeCompTable();
    PH_CHECK(hipMemcpyAsync(dComp.p, comp.c, 256, hipMemcpyHostToDevice, st));
    PH_CHECK(hipMemsetAsync(dRun.p, 0, 24, st));
    PH_CHECK(hipMemsetAsync((char *) o->d_data.p + capBytes, 0, 64, st));
    PH_CHECK(plasship::streamSync(st));          // (comp is a host static: the copy has completed before the host moves on anyway)

    // ---- batches: [PairMeta x n][big-pair list, padded to 16 bytes][records] packed on the host threads, one upload, then the kernels ----
    HostBytes hb; uint64_t hbCap = 0;
    bool kernelsPending = false;
    uint64_t nBigTotal = 0;
    for (uint64_t b0 = 0; b0 < N; b0 += batch) {
        const auto tp = std::chrono::steady_clock::now();
        const uint32_t n = (uint32_t) std::min<uint64_t>(batch, N - b0);
        std::vector<uint64_t> recOff(n + 1);
        std::vector<uint32_t> big;
        const uint64_t metaBytes = (uint64_t) n * sizeof(PairMeta);
        {
            uint64_t nb = 0;
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t l1 = recOf(b0 + k, 0).second->len, l2 = recOf(b0 + k, 1).second->len;
                recOff[k] = nb; nb += 2 * pad4(l1) + 2 * pad4(l2);
                if (l1 > MR_MAX_SMALL || l2 > MR_MAX_SMALL) big.push_back(k);
            }
            recOff[n] = nb;
        }
        const uint64_t bigBytes = (big.size() * 4 + 15) & ~15ull, recBase = metaBytes + bigBytes, total = recBase + recOff[n];
        if (total > hbCap) { if (!hb.alloc(total)) { setError("plasship_mergereads: out of host memory"); return PLASSHIP_ERR_IO; } hbCap = total; }
        PairMeta *meta = reinterpret_cast<PairMeta *>(hb.p);
        if (!big.empty()) memcpy(hb.p + metaBytes, big.data(), big.size() * 4);
        parallelRanges(n, [&](int, size_t kb, size_t ke) {
            for (size_t k = kb; k < ke; k++) {
                const auto r1 = recOf(b0 + k, 0), r2 = recOf(b0 + k, 1);
                const uint32_t l1 = r1.second->len, l2 = r2.second->len;
                meta[k].off = recBase + recOff[k]; meta[k].l1 = l1; meta[k].l2 = l2;
                char *d = hb.p + recBase + recOff[k];
                const uint64_t p1 = pad4(l1), p2 = pad4(l2);
                memcpy(d, r1.first->buf.p + r1.second->seq, l1); memset(d + l1, 0, p1 - l1);
                memcpy(d + p1, r1.first->buf.p + r1.second->qual, l1); memset(d + p1 + l1, 0, p1 - l1);
                memcpy(d + 2 * p1, r2.first->buf.p + r2.second->seq, l2); memset(d + 2 * p1 + l2, 0, p2 - l2);
                memcpy(d + 2 * p1 + p2, r2.first->buf.p + r2.second->qual, l2); memset(d + 2 * p1 + p2 + l2, 0, p2 - l2);
            }
        }, recOff.data(), 1024);
        msParse += msSince(tp);
        if (kernelsPending) {                     // the previous batch's kernels ran while this one was packed; its input buffer is reused
            PH_CHECK(hipEventSynchronize(ctx->ev[3]));
            float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); msKernel += ms;
            kernelsPending = false;
        }
        if (total > dPk.bytes && dPk.alloc(total) != hipSuccess) { setError("plasship_mergereads: out of device memory"); return PLASSHIP_ERR_DEVICE; }
        const auto tu = std::chrono::steady_clock::now();
        { const int rc = stagedCopyToDevice(ctx, dPk.p, hb.p, total); if (rc) return rc; }
        msUpload += msSince(tu);

        MergeArgs a;
        a.pk = dPk.as<char>(); a.meta = dPk.as<PairMeta>(); a.n = n; a.comp = dComp.as<unsigned char>();
        a.bigList = reinterpret_cast<const uint32_t *>(dPk.as<char>() + metaBytes); a.nBig = (uint32_t) big.size();
        a.status = dStatus.as<uint8_t>() + b0; a.pos = dPos.as<int32_t>(); a.nEnt = dEnt.as<uint32_t>(); a.nBytes = dBytes.as<uint64_t>();
        PH_CHECK(hipEventRecord(ctx->ev[2], st));
        const unsigned gridRows = (unsigned) std::min<uint64_t>((n + MR_ROWS - 1) / MR_ROWS, (uint64_t) ctx->numCU * 32);
        hipLaunchKernelGGL(mergePairsKernel, dim3(gridRows), dim3(256), 0, st, a);
        if (!big.empty()) hipLaunchKernelGGL(mergePairsWaveKernel, dim3((unsigned) std::min<uint64_t>((big.size() + 3) / 4, (uint64_t) ctx->numCU * 8)), dim3(256), 0, st, a);
        if (exclusiveScanU32(st, dEnt.as<uint32_t>(), dEntBase.as<uint64_t>(), n, dTmp.p, tmpBytes) ||
            exclusiveScanU64(st, dBytes.as<uint64_t>(), dByteBase.as<uint64_t>(), n, dTmp.p, tmpBytes)) { setError("plasship_mergereads: scan failed"); return PLASSHIP_ERR_DEVICE; }
        WriteArgs w;
        w.pk = a.pk; w.meta = a.meta; w.n = n; w.comp = a.comp; w.status = a.status; w.pos = a.pos;
        w.entBase = dEntBase.as<uint64_t>(); w.byteBase = dByteBase.as<uint64_t>(); w.run = dRun.as<uint64_t>();
        w.data = o->d_data.as<char>(); w.off = o->d_off.as<uint64_t>(); w.len = o->d_len.as<uint32_t>(); w.key = o->d_key.as<uint32_t>();
        w.maxLen = reinterpret_cast<uint32_t *>(dRun.as<uint64_t>() + 2);
        hipLaunchKernelGGL(mergeWriteKernel, dim3((unsigned) std::min<uint64_t>((n + 15) / 16, (uint64_t) ctx->numCU * 32)), dim3(256), 0, st, w);
        hipLaunchKernelGGL(mergeRunKernel, dim3(1), dim3(64), 0, st, dRun.as<uint64_t>(), w.entBase, w.byteBase, n);
        PH_CHECK(hipEventRecord(ctx->ev[3], st));
        PH_CHECK(hipGetLastError());
        kernelsPending = true;
        nBigTotal += big.size();
    }
    uint64_t run[3] = {0, 0, 0};
    PH_COPY_SYNC(st, run, dRun.p, 24, hipMemcpyDeviceToHost);
    PH_CHECK(hipGetLastError());
    if (kernelsPending) { float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); msKernel += ms; }
    const uint64_t nOut = run[0], dataBytes = run[1];
    if (dataBytes > capBytes || nOut > 2 * N) { setError("plasship_mergereads: internal error (output beyond its bound)"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemcpyAsync(o->d_off.as<uint64_t>() + nOut, &dataBytes, 8, hipMemcpyHostToDevice, st));
    o->dbtype = PLASSHIP_DBTYPE_NUCLEOTIDES; o->n = (size_t) nOut; o->dataBytes = dataBytes; o->residues = dataBytes - 2 * nOut;
    o->maxEntryLen = nOut ? (uint32_t) run[2] + 2 : 0; o->hostIndexValid = false;

    // ---- header DB on the host (mergereads.cpp:87-114: mate 1's name for a merged pair, mate 1's and mate 2's for an unmerged one) ----
    const auto th0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> status(N + 1);
    if (N) { const int rc = stagedCopyToHost(ctx, status.data(), dStatus.p, N); if (rc) return rc; }
    std::unique_ptr<plasship_seqdb> h(new plasship_seqdb());
    h->h_key.resize(nOut); h->h_elen.resize(nOut); h->h_off.resize(nOut + 1);
    std::vector<uint64_t> pairEnt(N + 1, 0), pairBytes(N + 1, 0);
    for (uint64_t p = 0; p < N; p++) {
        const uint32_t n1 = recOf(p, 0).second->nameLen;
        pairEnt[p + 1] = pairEnt[p] + (status[p] ? 1 : 2);
        pairBytes[p + 1] = pairBytes[p] + n1 + 2 + (status[p] ? 0 : recOf(p, 1).second->nameLen + 2);
    }
    if (pairEnt[N] != nOut) { setError("plasship_mergereads: internal error (entry counts of the two DBs differ)"); return PLASSHIP_ERR_DEVICE; }
    const uint64_t hBytes = pairBytes[N];
    HostBytes hd;
    if (!hd.alloc(hBytes)) { setError("plasship_mergereads: out of host memory"); return PLASSHIP_ERR_IO; }
    std::atomic<uint32_t> hMax(0);
    parallelRanges((size_t) N, [&](int, size_t pb, size_t pe) {
        uint32_t mx = 0;
        for (size_t p = pb; p < pe; p++) {
            uint64_t e = pairEnt[p], b = pairBytes[p];
            for (int mate = 0; mate < (status[p] ? 1 : 2); mate++, e++) {
                const auto r = recOf(p, mate);
                memcpy(hd.p + b, r.first->buf.p + r.second->name, r.second->nameLen);
                hd.p[b + r.second->nameLen] = '\n'; hd.p[b + r.second->nameLen + 1] = 0;
                h->h_key[e] = (uint32_t) e; h->h_elen[e] = r.second->nameLen + 2; h->h_off[e] = b;
                b += r.second->nameLen + 2; mx = std::max(mx, r.second->nameLen);
            }
        }
        uint32_t cur = hMax.load();
        while (mx > cur && !hMax.compare_exchange_weak(cur, mx)) {}
    }, pairEnt.data(), 4096);
    h->h_off[nOut] = hBytes;
    std::vector<uint32_t> hLen(nOut);
    for (uint64_t e = 0; e < nOut; e++) hLen[e] = h->h_elen[e] - 2;
    if (h->d_data.allocLong(hBytes + 64) != hipSuccess || h->d_off.allocLong((nOut + 1) * 8) != hipSuccess || h->d_len.allocLong((nOut + 1) * 4) != hipSuccess ||
        h->d_key.allocLong((nOut + 1) * 4) != hipSuccess) { setError("plasship_mergereads: out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync((char *) h->d_data.p + hBytes, 0, 64, st));
    int rc = stagedCopyToDevice(ctx, h->d_data.p, hd.p, hBytes); if (rc) return rc;
    rc = stagedCopyToDevice(ctx, h->d_off.p, h->h_off.data(), (nOut + 1) * 8); if (rc) return rc;
    rc = stagedCopyToDevice(ctx, h->d_len.p, hLen.data(), nOut * 4); if (rc) return rc;
    rc = stagedCopyToDevice(ctx, h->d_key.p, h->h_key.data(), nOut * 4); if (rc) return rc;
    h->h_off.resize(nOut);
    h->dbtype = 12;             // Parameters::DBTYPE_GENERIC_DB (mm/commons/Parameters.h:77)
    h->n = (size_t) nOut; h->dataBytes = hBytes; h->residues = hBytes - 2 * nOut; h->maxEntryLen = nOut ? hMax.load() + 2 : 0; h->hostIndexValid = true;
    PH_CHECK(plasship::streamSync(st));
    msParse += msSince(th0);
    if (stats) {
        uint64_t comb = 0; for (uint64_t p = 0; p < N; p++) comb += status[p];
        stats->pairs = N; stats->combined = comb; stats->not_combined = N - comb;
        stats->ms_parse = (float) msParse; stats->ms_upload = (float) msUpload; stats->ms_kernel = (float) msKernel;
        stats->long_pairs = nBigTotal;
    }
    *reads = o.release();
    *headers = h.release();
    return PLASSHIP_OK;
}
