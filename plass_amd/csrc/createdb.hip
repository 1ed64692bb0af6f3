// plasship: createdb for reads — FASTQ / FASTA files -> read DB + header DB (replaces int createdb(int, const char**, const Command&),
// lib/mmseqs/src/util/createdb.cpp:15-333, with kseq as its parser, lib/mmseqs/lib/ksw2/kseq.h:96-233).  Product code.
//
//   host    reads a file (plain: pread on the host threads; .gz: one zlib stream — host_util.cpp, shared with mergereads) and hands the raw
//           bytes to the device in chunks through the context's pinned double buffer (PLASSHIP_TUNE_FASTQ_CHUNK_KB; default: a staging
//           buffer).  Nothing is parsed on the host.
//   device  per file, on the raw bytes as they lie in HBM (a file's buffer is padded with zero bytes to whole 4 KB tiles, a final line
//           without '\n' gets one):
//             newlineKernel<0>   per 4 KB tile (256 lanes x 16 bytes, SWAR zero-byte test on the bytes ^ '\n', popcount, wave + block
//                                reduction) the number of newlines.  Runs per chunk, under the copy of the next one, on the tiles that chunk
//                                completed; a tile — and with it every line and record — that straddles a chunk boundary stays where it is
//                                on the device and is taken with the chunk that completes it.
//             newlineKernel<1>   scan of the tile counts, then the same test again writes every newline's position (count, then write: the
//                                idiom of orfKernel<PASS>; no atomics)
//             lineKernel         one 16-lane row per line: what the line is (FASTQ: by its number mod 4; FASTA: '>' opens a record), its
//                                length as kseq leaves it ('\r' before '\n' dropped when the line holds more), name / comment split at the
//                                first isspace() byte, the FASTQ checks ('@', '+', equal lengths, quality < 128); the first offence goes
//                                back as (line << 8 | code)
//             scans (scan.hip)   headers before a line = its record; sequence bytes before a line = its place inside the record
//             scatterKernel      lengths into KEY order: key = rank of (id_offset + i) % 32's split + i / 32 (createdb.cpp:60,219,275-277)
//             scans              entry offsets of the read DB and the header DB in key order
//             writeKernel        one 16-lane row per LINE: a sequence line goes to its place in its entry (dword stores on the aligned
//                                destination, the source funnel-shifted), a header line writes the header entry and both terminators
//           A multi-line FASTA entry is therefore a stream compaction at line granularity; nothing is special about long entries except that
//           ONE row copies a line, so single lines of megabytes run at a fraction of the bandwidth (no cut: they are correct, only slower).
#include "common.hpp"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <unistd.h>
#include <vector>

namespace plasship {

constexpr int CD_TILE = 4096;             // bytes per workgroup round
constexpr uint32_t CD_NONE = 0xFFFFFFFFu;
enum { CD_FASTQ = 0, CD_FASTA = 1 };
// what lineKernel reports (the smallest line wins)
enum { CDE_NO_AT = 1, CDE_NO_PLUS = 2, CDE_QUAL_LEN = 3, CDE_QUAL_BYTE = 4, CDE_NO_NAME = 5, CDE_SEQ_START = 6, CDE_FASTA_MIXED = 8, CDE_FASTA_CR = 9, CDE_TOO_LONG = 10 };

// bit k set: byte k of the 16 is '\n' (exact zero-byte test on x ^ "\n\n\n\n": no carry leaves a byte)
__device__ __forceinline__ uint32_t newlineMask16(const uint4 w) {
    const uint32_t v[4] = {w.x, w.y, w.z, w.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t y = v[j] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);      // 0x80 in every zero byte
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * j);
    }
    return m;
}

// PASS 0: tileCnt[t] = newlines of tile t, tiles [t0, t1).  PASS 1: their positions to nl[tileBase[t] ..).
template <int PASS>
__global__ __launch_bounds__(256) void newlineKernel(const uint4 *__restrict__ raw, uint64_t t0, uint64_t t1, uint32_t *__restrict__ tileCnt,
                                                     const uint64_t *__restrict__ tileBase, uint64_t *__restrict__ nl) {
    __shared__ uint32_t part[4];
    const int wv = threadIdx.x >> 6;
    for (uint64_t t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
        const uint32_t m = newlineMask16(raw[t * 256 + threadIdx.x]);
        const uint32_t c = (uint32_t) __popc(m);
        const uint32_t inc = waveInclusiveScan(c);
        __syncthreads();                                      // part[] of the previous round read
        if (laneId() == 63) part[wv] = inc;
        __syncthreads();
        if (PASS == 0) { if (threadIdx.x == 0) tileCnt[t] = part[0] + part[1] + part[2] + part[3]; }
        else {
            uint64_t o = tileBase[t] + (inc - c);
            for (int k = 0; k < wv; k++) o += part[k];
            const uint64_t b = t * CD_TILE + (uint64_t) threadIdx.x * 16;
            for (uint32_t r = m; r; r &= r - 1) nl[o++] = b + (uint32_t) (__ffs((int) r) - 1);
        }
    }
}

__device__ __forceinline__ bool kseqIsSpace(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

struct LineArgs {
    const unsigned char *raw; const uint64_t *nl; uint64_t nLines; int fmt;
    uint32_t *isHdr, *contrib, *hName, *hLen;               // [nLines]: 1 for a header line; sequence bytes of a sequence line; name / header length of a header line
    unsigned long long *err;                                // min over (line << 8 | code)
};
// one 16-lane row per line
__global__ __launch_bounds__(256) void lineKernel(LineArgs a) {
    const int l = threadIdx.x & 15;
    const uint64_t row0 = ((uint64_t) blockIdx.x * 256 + threadIdx.x) >> 4, nRows = ((uint64_t) gridDim.x * 256) >> 4;
    for (uint64_t line = row0; line < a.nLines; line += nRows) {
        const uint64_t start = line ? a.nl[line - 1] + 1 : 0, end = a.nl[line], rawLen = end - start;
        const unsigned char first = rawLen ? a.raw[start] : 0, last = rawLen ? a.raw[end - 1] : 0;
        const uint64_t len = rawLen - ((rawLen > 1 && last == '\r') ? 1 : 0);          // kseq.h:145
        int code = 0;
        if (rawLen > 0x7FFFFFF0ull) code = CDE_TOO_LONG;
        const int q = (int) (line & 3);
        const bool hdr = a.fmt == CD_FASTQ ? q == 0 : first == '>';
        const bool seq = a.fmt == CD_FASTQ ? q == 1 : !hdr;
        uint32_t nameLen = 0, hdrLen = 0;
        if (hdr && !code) {
            if (a.fmt == CD_FASTQ && first != '@') code = CDE_NO_AT;
            const uint64_t body = rawLen ? rawLen - 1 : 0;                           // bytes behind '@' / '>'
            uint32_t found = CD_NONE;
            for (uint64_t j0 = 0; j0 < body && found == CD_NONE; j0 += 16) {         // row-uniform trip count
                const uint64_t j = j0 + l;
                const bool sp = j < body && kseqIsSpace(a.raw[start + 1 + j]);
                found = rowMin16U32(sp ? (uint32_t) j : CD_NONE);
            }
            nameLen = found == CD_NONE ? (uint32_t) body : found;
            // kseq.h:199-200: the byte that ended the name is dropped; unless it was the '\n', the rest of the line is the comment
            uint64_t cmt = found == CD_NONE ? 0 : body - nameLen - 1;
            if (cmt > 1 && last == '\r') cmt--;
            hdrLen = cmt ? nameLen + 1 + (uint32_t) cmt : nameLen;                    // createdb.cpp:161-165: name [' ' comment]
            if (!code && nameLen == 0) code = CDE_NO_NAME;
        } else if (seq && !code) {
            if (a.fmt == CD_FASTQ) { if (first == '>' || first == '@' || first == '+') code = CDE_SEQ_START; }
            else if (first == '@' || first == '+') code = CDE_FASTA_MIXED;
            else if (rawLen == 1 && first == '\r') code = CDE_FASTA_CR;
        } else if (a.fmt == CD_FASTQ && q == 2 && !code) {
            if (first != '+') code = CDE_NO_PLUS;
        } else if (a.fmt == CD_FASTQ && q == 3 && !code) {
            const uint64_t s2 = a.nl[line - 3] + 1, e2 = a.nl[line - 2], r2 = e2 - s2;
            const uint64_t l2 = r2 - ((r2 > 1 && a.raw[e2 - 1] == '\r') ? 1 : 0);
            uint32_t hi = 0;
            for (uint64_t j = l; j < len; j += 16) hi |= a.raw[start + j];
            hi = rowOr16(hi);
            if (l2 != len) code = CDE_QUAL_LEN; else if (hi & 0x80u) code = CDE_QUAL_BYTE;
        }
        if (l == 0) {
            a.isHdr[line] = hdr ? 1u : 0u; a.contrib[line] = seq ? (uint32_t) len : 0u; a.hName[line] = nameLen; a.hLen[line] = hdrLen;
            if (code) atomicMin(a.err, (unsigned long long) ((line << 8) | (uint64_t) code));
        }
    }
}

// per record (a header line): where its sequence bytes start in the file's run of sequence bytes, the header's lengths
__global__ __launch_bounds__(256) void recordKernel(const uint32_t *__restrict__ isHdr, const uint64_t *__restrict__ hdrScan, const uint64_t *__restrict__ seqPrefix,
                                                    const uint32_t *__restrict__ hName, const uint32_t *__restrict__ hLen, uint64_t nLines, uint64_t nRec,
                                                    uint64_t *__restrict__ recSeqStart, uint32_t *__restrict__ recName, uint32_t *__restrict__ recHdr) {
    for (uint64_t line = (uint64_t) blockIdx.x * 256 + threadIdx.x; line < nLines; line += (uint64_t) gridDim.x * 256) {
        if (!isHdr[line]) continue;
        const uint64_t r = hdrScan[line];
        recSeqStart[r] = seqPrefix[line]; recName[r] = hName[line]; recHdr[r] = hLen[line];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) recSeqStart[nRec] = seqPrefix[nLines];
}

// the shuffle (createdb.cpp:60,219: entry id goes to split id % 32; DBWriter::createRenumberedDB, :275-277, numbers the merged file through)
struct KeyMap { uint32_t splits, idOffset, renumber; uint32_t splitBase[32]; };
__host__ __device__ inline uint32_t keyRank(const KeyMap &k, uint64_t g) {              // position of input entry g in the data file
    const uint32_t S = k.splits, s = (uint32_t) ((k.idOffset + g) % S), i0 = (s + S - k.idOffset % S) % S;
    return k.splitBase[s] + (uint32_t) ((g - i0) / S);
}

// residues of the sampled entries that are one of ACGTUN in either case (createdb.cpp:176-197); probe[2g] += count, probe[2g + 1] += length
__global__ __launch_bounds__(256) void probeKernel(const unsigned char *__restrict__ raw, const uint64_t *__restrict__ nl, uint64_t nLines, const uint32_t *__restrict__ contrib,
                                                   const uint64_t *__restrict__ hdrScan, uint64_t recBase, uint64_t nSample, unsigned long long *__restrict__ probe) {
    const int l = threadIdx.x & 15;
    const uint64_t row0 = ((uint64_t) blockIdx.x * 256 + threadIdx.x) >> 4, nRows = ((uint64_t) gridDim.x * 256) >> 4;
    for (uint64_t line = row0; line < nLines; line += nRows) {
        const uint32_t n = contrib[line];
        const uint64_t h = hdrScan[line];                     // headers before this line; a sequence line belongs to record h - 1
        if (!n || !h || recBase + h - 1 >= nSample) continue;
        const uint64_t start = line ? nl[line - 1] + 1 : 0;
        int c = 0;
        for (uint32_t j = l; j < n; j += 16) {
            const unsigned char x = raw[start + j] & 0xDFu;   // toupper for letters; no other byte maps onto one of the six
            c += (x == 'A' || x == 'C' || x == 'G' || x == 'T' || x == 'U' || x == 'N') ? 1 : 0;
        }
        c = rowSum16(c);
        if (l == 0) { atomicAdd(&probe[2 * (recBase + h - 1)], (unsigned long long) c); atomicAdd(&probe[2 * (recBase + h - 1) + 1], (unsigned long long) n); }
    }
}

struct ScatterArgs {
    const uint64_t *recSeqStart; const uint32_t *recHdr; uint64_t nRec, recBase; uint32_t fileNo; KeyMap km;
    uint32_t *seqLenK, *seqEntK, *hdrLenK, *hdrEntK, *keyK; uint16_t *fileK;    // [N], key order
    unsigned long long *maxLen;                                                  // [0] longest sequence, [1] longest header
};
__global__ __launch_bounds__(256) void scatterKernel(ScatterArgs a) {
    for (uint64_t r = (uint64_t) blockIdx.x * 256 + threadIdx.x; r < a.nRec; r += (uint64_t) gridDim.x * 256) {
        const uint64_t len = a.recSeqStart[r + 1] - a.recSeqStart[r];
        const uint32_t k = keyRank(a.km, a.recBase + r), hl = a.recHdr[r];
        const uint32_t l32 = (uint32_t) (len > 0x7FFFFFF0ull ? 0x7FFFFFF0ull : len);
        a.seqLenK[k] = l32; a.seqEntK[k] = l32 + 2; a.hdrLenK[k] = hl; a.hdrEntK[k] = hl + 2;
        a.keyK[k] = a.km.renumber ? k : a.km.idOffset + k; a.fileK[k] = (uint16_t) a.fileNo;
        atomicMax(&a.maxLen[0], (unsigned long long) len); atomicMax(&a.maxLen[1], (unsigned long long) hl);
    }
}

// n bytes src -> dst by one row of 16 lanes: bytes up to the first 4-byte boundary of dst, dwords (two aligned source dwords funnel-shifted:
// the source buffer is padded, the dword behind its last byte may be read), the last bytes.  Byte `patch` (CD_NONE: none) becomes ' '; it is
// replaced in the value that is stored, so no two lanes write one byte.
__device__ __forceinline__ void rowCopy(unsigned char *dst, const unsigned char *src, uint32_t n, int l, uint32_t patch) {
    const uint32_t head = min(n, (uint32_t) ((4 - ((uintptr_t) dst & 3)) & 3));
    if ((uint32_t) l < head) dst[l] = (uint32_t) l == patch ? (unsigned char) ' ' : src[l];
    const uint32_t words = (n - head) >> 2;
    const unsigned char *s = src + head; uint32_t *d = reinterpret_cast<uint32_t *>(dst + head);
    const uint32_t sh = (uint32_t) ((uintptr_t) s & 3);
    const uint32_t *sa = reinterpret_cast<const uint32_t *>(s - sh);
    for (uint32_t w = l; w < words; w += 16) {
        const uint32_t lo = sa[w], hi = sh ? sa[w + 1] : 0u;
        uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh);
        const uint32_t pb = patch - (head + 4 * w);            // wraps for CD_NONE and for a byte before this dword
        if (pb < 4) v = (v & ~(0xFFu << (8 * pb))) | (0x20u << (8 * pb));
        d[w] = v;
    }
    const uint32_t t = head + 4 * words + (uint32_t) l;
    if (t < n) dst[t] = t == patch ? (unsigned char) ' ' : src[t];          // at most 3 bytes
}

struct WriteArgs {
    const unsigned char *raw; const uint64_t *nl; uint64_t nLines;
    const uint32_t *isHdr, *contrib; const uint64_t *hdrScan, *seqPrefix;
    const uint64_t *recSeqStart; const uint32_t *recName, *recHdr; uint64_t recBase; KeyMap km;
    const uint64_t *seqOff, *hdrOff;                         // [N + 1] entry offsets in key order
    unsigned char *seqData, *hdrData;
};
// one 16-lane row per line: a sequence line to its place inside its entry; a header line writes the header entry ("name[ comment]\n\0")
// and the "\n\0" of the sequence entry
__global__ __launch_bounds__(256) void writeKernel(WriteArgs a) {
    const int l = threadIdx.x & 15;
    const uint64_t row0 = ((uint64_t) blockIdx.x * 256 + threadIdx.x) >> 4, nRows = ((uint64_t) gridDim.x * 256) >> 4;
    for (uint64_t line = row0; line < a.nLines; line += nRows) {
        const uint64_t start = line ? a.nl[line - 1] + 1 : 0;
        if (a.isHdr[line]) {
            const uint64_t r = a.hdrScan[line];
            const uint32_t k = keyRank(a.km, a.recBase + r), hl = a.recHdr[r], nm = a.recName[r];
            unsigned char *h = a.hdrData + a.hdrOff[k];
            rowCopy(h, a.raw + start + 1, hl, l, hl > nm ? nm : CD_NONE);      // kseq drops the byte that ended the name, createdb puts ' ' (a tab becomes a blank)
            if (l == 0) {
                h[hl] = '\n'; h[hl + 1] = 0;
                unsigned char *e = a.seqData + a.seqOff[k + 1] - 2;
                e[0] = '\n'; e[1] = 0;
            }
        } else if (const uint32_t n = a.contrib[line]) {
            const uint64_t r = a.hdrScan[line] - 1;           // (a sequence line is behind its header: hdrScan >= 1; checked on the host for line 0)
            const uint32_t k = keyRank(a.km, a.recBase + r);
            rowCopy(a.seqData + a.seqOff[k] + (a.seqPrefix[line] - a.recSeqStart[r]), a.raw + start, n, l, CD_NONE);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static double msSinceCd(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

struct CdFile {
    std::string path; int fmt = CD_FASTQ; uint64_t bytes = 0, nLines = 0, nRec = 0, recBase = 0;
    DevBuf raw, nl, isHdr, contrib, hdrScan, seqPrefix, recSeqStart, recName, recHdr;
};

// Util::parseFastaHeader (lib/mmseqs/src/commons/Util.cpp:173-256) on a header's first word: the identifier a .lookup line carries
static std::string lookupName(const std::string &header) {
    if (header.empty()) return "";
    size_t offset = 0;
    if (header.compare(0, 10, "consensus_") == 0) offset = 10;
    static const struct { const char *prefix; unsigned length, bar; } dbs[] = {{"uc", 2, 0}, {"cl|", 3, 1}, {"sp|", 3, 1}, {"tr|", 3, 1}, {"gb|", 3, 1},
        {"ref|", 4, 1}, {"pdb|", 4, 1}, {"bbs|", 4, 1}, {"lcl|", 4, 1}, {"pir||", 5, 1}, {"prf||", 5, 1}, {"gnl|", 4, 2}, {"pat|", 4, 2}, {"gi|", 3, 3}};
    for (const auto &d : dbs) {
        if (header.compare(offset, strlen(d.prefix), d.prefix) != 0 || header.size() < offset + strlen(d.prefix)) continue;
        size_t start = offset + d.length;
        for (unsigned j = 0; d.bar > 1 && j < d.bar - 1; j++) {
            const size_t end = header.find('|', start);
            if (end == std::string::npos) return "";
            start = end + 1;
        }
        size_t end = header.find('|', start);
        if (end == std::string::npos) end = header.find_first_of(" \n", start);
        if (end == std::string::npos) end = header.size();
        return start <= end ? header.substr(start, end - start) : "";
    }
    size_t end = header.find_first_of(" \n", offset);
    if (end == std::string::npos) end = header.size();
    return header.substr(offset, end - offset);
}

static bool writeWholeFile(const std::string &path, const std::string &bytes, std::string &err) {
    const std::string tmp = path + ".tmp." + std::to_string((long) getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot open " + tmp + " for writing"; return false; }
    const bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); err = "cannot write " + path; return false; }
    return true;
}

// a FASTQ record whose third line is not a '+' line: more sequence lines up to a '+' line (multi-line FASTQ, which kseq reads), or a
// record that has none before the next '@' line / the end of the file (broken)
static bool looksMultiLine(const HostBytes &buf, uint64_t recStartLine) {
    const char *B = buf.p; const uint64_t S = buf.n;
    uint64_t p = 0, line = 0;
    while (p < S && line < recStartLine + 2) { const void *q = memchr(B + p, '\n', S - p); if (!q) return false; p = (uint64_t) ((const char *) q - B) + 1; line++; }
    while (p < S) {
        if (B[p] == '+') return true;
        if (B[p] == '@') return false;
        const void *q = memchr(B + p, '\n', S - p); if (!q) return false; p = (uint64_t) ((const char *) q - B) + 1;
    }
    return false;
}

static int createdbImpl(plasship_ctx *ctx, const char *const *files, size_t n_files, const plasship_createdb_params *par, const char *dbPath,
                        plasship_seqdb **outReads, plasship_createdb_stats *stats) {
    const char *W = "plasship_createdb: ";
    if (!ctx || !files || !n_files || (!outReads && !dbPath)) { setError(std::string(W) + "bad argument (at least one file, and an output)"); return PLASSHIP_ERR_ARG; }
    for (size_t k = 0; k < n_files; k++) if (!files[k]) { setError(std::string(W) + "NULL file name"); return PLASSHIP_ERR_ARG; }
    plasship_createdb_params P; P.shuffle = 1; P.id_offset = 0; P.dbtype = 0;
    if (par) P = *par;
    if (P.dbtype < 0 || P.dbtype > 2) { setError(std::string(W) + "dbtype must be 0 (auto), 1 or 2"); return PLASSHIP_ERR_ARG; }
    if (P.dbtype == 1) { setError(std::string(W) + "amino-acid input is not an input of the assembly workflows (left to the reference)"); return PLASSHIP_ERR_UNSUPPORTED; }
    if (n_files > 65535) { setError(std::string(W) + "more than 65535 files"); return PLASSHIP_ERR_UNSUPPORTED; }      // .lookup's file number is an unsigned short (createdb.cpp:78)
    // KSeqFactory (KSeqWrapper.cpp:160-195): "stdin" and .bz2 are left to the reference
    for (size_t k = 0; k < n_files; k++) {
        const std::string p = files[k];
        if (p == "stdin") { setError(std::string(W) + "reading stdin is left to the reference"); return PLASSHIP_ERR_UNSUPPORTED; }
        if (pathEndsWith(p, ".bz2")) { setError(std::string(W) + p + ": bzip2 input is left to the reference"); return PLASSHIP_ERR_UNSUPPORTED; }
    }
    PH_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const auto tAll = std::chrono::steady_clock::now();
    double msRead = 0, msUpload = 0, msKernel = 0, msWrite = 0;
    uint64_t chunks = 0, bytesIn = 0, linesAll = 0;
    const uint64_t chunkBytes = (uint64_t) tuneInt("FASTQ_CHUNK_KB", 0) << 10;          // 0: a staging buffer
    const unsigned grid = (unsigned) ctx->numCU * 8;
    auto kernelsBegin = [&]() { return hipEventRecord(ctx->ev[2], st); };
    auto kernelsEnd = [&](double &acc) -> int {               // waits: every caller needs what the kernels wrote on the host next
        PH_CHECK(hipEventRecord(ctx->ev[3], st)); PH_CHECK(hipGetLastError()); PH_CHECK(plasship::streamSync(st));
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]); acc += ms; return PLASSHIP_OK;
    };
    DevBuf dErr, dTmp, dProbe, dMax;
    if (dErr.alloc(8) != hipSuccess || dProbe.alloc(20 * 8) != hipSuccess || dMax.alloc(16) != hipSuccess) { setError(std::string(W) + "out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync(dProbe.p, 0, 20 * 8, st)); PH_CHECK(hipMemsetAsync(dMax.p, 0, 16, st));
    const uint64_t nSample = P.dbtype == 0 ? 10 : 0;           // createdb.cpp:177: sampleCount stops counting at 10, so the first ten entries are the sample

    std::vector<std::unique_ptr<CdFile>> F;
    uint64_t N = 0;
    for (size_t fi = 0; fi < n_files; fi++) {
        F.emplace_back(new CdFile()); CdFile &f = *F.back(); f.path = files[fi]; f.recBase = N;
        HostBytes hb; std::string err;
        const auto tr = std::chrono::steady_clock::now();
        if (!readSeqFileBytes(f.path, hb, err)) { setError(std::string(W) + err); return PLASSHIP_ERR_IO; }
        msRead += msSinceCd(tr);
        const uint64_t S = hb.n; f.bytes = S; bytesIn += S;
        if (S == 0) continue;                                  // kseq finds no entry
        if (hb.p[0] == '@') f.fmt = CD_FASTQ; else if (hb.p[0] == '>') f.fmt = CD_FASTA;
        else { setError(std::string(W) + f.path + ": does not start with '@' or '>' (kseq's search for the first header is left to the reference)"); return PLASSHIP_ERR_UNSUPPORTED; }
        const bool addNl = hb.p[S - 1] != '\n';                // a final line without '\n' is a line (kseq.h:105-113)
        const uint64_t nTiles = (S + (addNl ? 1 : 0) + CD_TILE - 1) / CD_TILE, padded = nTiles * CD_TILE + 16;
        DevBuf tileCnt, tileBase;
        const size_t tmpNeed = exclusiveScanTmpBytes((size_t) nTiles + 1);
        if (f.raw.alloc(padded) != hipSuccess || tileCnt.alloc((nTiles + 1) * 4) != hipSuccess || tileBase.alloc((nTiles + 2) * 8) != hipSuccess ||
            (tmpNeed > dTmp.bytes && dTmp.alloc(tmpNeed) != hipSuccess)) { setError(std::string(W) + "out of device memory"); return PLASSHIP_ERR_DEVICE; }
        // ---- upload in chunks; the newline count of the tiles a chunk completed runs while the next chunk is produced and copied ----
        const auto tu = std::chrono::steady_clock::now();
        PH_CHECK(hipMemsetAsync(f.raw.as<char>() + S, 0, padded - S, st));
        if (addNl) PH_CHECK(hipMemsetAsync(f.raw.as<char>() + S, '\n', 1, st));
        uint64_t tilesDone = 0;
        const std::function<int(uint64_t)> counted = [&](uint64_t end) -> int {
            chunks++;
            const uint64_t t1 = end >= S ? nTiles : end / CD_TILE;      // the tile a chunk ends in waits for the chunk that completes it
            if (t1 > tilesDone) {
                hipLaunchKernelGGL(newlineKernel<0>, dim3((unsigned) std::min<uint64_t>(t1 - tilesDone, grid)), dim3(256), 0, st, f.raw.as<uint4>(), tilesDone, t1,
                                   tileCnt.as<uint32_t>(), (const uint64_t *) nullptr, (uint64_t *) nullptr);
                tilesDone = t1;
            }
            return hipGetLastError() == hipSuccess ? PLASSHIP_OK : PLASSHIP_ERR_DEVICE;
        };
        { const int rc = stagedUpload(ctx, f.raw.p, S, [&](char *dst, uint64_t o, uint64_t n) {
            const size_t SL = 1u << 20;
            parallelRanges((size_t) ((n + SL - 1) / SL), [&](int, size_t b, size_t e) { const uint64_t x = (uint64_t) b * SL, y = std::min<uint64_t>(n, (uint64_t) e * SL); if (y > x) memcpy(dst + x, hb.p + o + x, (size_t) (y - x)); }, nullptr, 4);
        }, chunkBytes, &counted); if (rc) { if (rc == PLASSHIP_ERR_DEVICE) setError(std::string(W) + "newline kernel launch failed"); return rc; } }
        msUpload += msSinceCd(tu);
        // ---- lines ----
        PH_CHECK(kernelsBegin());
        if (exclusiveScanU32(st, tileCnt.as<uint32_t>(), tileBase.as<uint64_t>(), nTiles, dTmp.p, dTmp.bytes)) { setError(std::string(W) + "scan failed"); return PLASSHIP_ERR_DEVICE; }
        uint64_t nLines = 0;
        PH_CHECK(hipMemcpyAsync(&nLines, tileBase.as<uint64_t>() + nTiles, 8, hipMemcpyDeviceToHost, st));
        { const int rc = kernelsEnd(msKernel); if (rc) return rc; }
        f.nLines = nLines; linesAll += nLines;
        if (nLines == 0 || nLines > S + 1) { setError(std::string(W) + "internal error (line count)"); return PLASSHIP_ERR_DEVICE; }
        const size_t tmpL = exclusiveScanTmpBytes((size_t) nLines + 1);
        DevBuf hName, hLen;
        if (f.nl.alloc(nLines * 8) != hipSuccess || f.isHdr.alloc((nLines + 1) * 4) != hipSuccess || f.contrib.alloc((nLines + 1) * 4) != hipSuccess ||
            hName.alloc(nLines * 4) != hipSuccess || hLen.alloc(nLines * 4) != hipSuccess || f.hdrScan.alloc((nLines + 2) * 8) != hipSuccess ||
            f.seqPrefix.alloc((nLines + 2) * 8) != hipSuccess || (tmpL > dTmp.bytes && dTmp.alloc(tmpL) != hipSuccess)) { setError(std::string(W) + "out of device memory"); return PLASSHIP_ERR_DEVICE; }
        const unsigned long long noErr = ~0ull;
        PH_CHECK(hipMemcpyAsync(dErr.p, &noErr, 8, hipMemcpyHostToDevice, st));
        PH_CHECK(kernelsBegin());
        hipLaunchKernelGGL(newlineKernel<1>, dim3((unsigned) std::min<uint64_t>(nTiles, grid)), dim3(256), 0, st, f.raw.as<uint4>(), (uint64_t) 0, nTiles, (uint32_t *) nullptr,
                           tileBase.as<uint64_t>(), f.nl.as<uint64_t>());
        LineArgs la; la.raw = f.raw.as<unsigned char>(); la.nl = f.nl.as<uint64_t>(); la.nLines = nLines; la.fmt = f.fmt;
        la.isHdr = f.isHdr.as<uint32_t>(); la.contrib = f.contrib.as<uint32_t>(); la.hName = hName.as<uint32_t>(); la.hLen = hLen.as<uint32_t>(); la.err = dErr.as<unsigned long long>();
        const unsigned gridRows = (unsigned) std::min<uint64_t>((nLines + 15) / 16, (uint64_t) grid * 4);
        hipLaunchKernelGGL(lineKernel, dim3(gridRows), dim3(256), 0, st, la);
        if (exclusiveScanU32(st, f.isHdr.as<uint32_t>(), f.hdrScan.as<uint64_t>(), nLines, dTmp.p, dTmp.bytes) ||
            exclusiveScanU32(st, f.contrib.as<uint32_t>(), f.seqPrefix.as<uint64_t>(), nLines, dTmp.p, dTmp.bytes)) { setError(std::string(W) + "scan failed"); return PLASSHIP_ERR_DEVICE; }
        unsigned long long e = 0; uint64_t nRec = 0;
        PH_CHECK(hipMemcpyAsync(&e, dErr.p, 8, hipMemcpyDeviceToHost, st));
        PH_CHECK(hipMemcpyAsync(&nRec, f.hdrScan.as<uint64_t>() + nLines, 8, hipMemcpyDeviceToHost, st));
        { const int rc = kernelsEnd(msKernel); if (rc) return rc; }
        // ---- refusals: before anything exists ----
        if (e != noErr) {
            const uint64_t line = e >> 8; const int code = (int) (e & 0xFF);
            const std::string where = f.path + (f.fmt == CD_FASTQ ? ": record " + std::to_string(line / 4 + 1) : ": line " + std::to_string(line + 1)) + ": ";
            int rc = PLASSHIP_ERR_IO; std::string why;
            switch (code) {
            case CDE_NO_AT: why = "a record does not start with '@'"; break;
            case CDE_NO_PLUS:
                if (looksMultiLine(hb, line - 2)) { why = "multi-line sequence (read by the reference)"; rc = PLASSHIP_ERR_UNSUPPORTED; }
                else why = "a missing '+' line";
                break;
            case CDE_QUAL_LEN: why = "a quality string whose length differs from the sequence's"; break;
            case CDE_QUAL_BYTE: why = "a quality byte >= 128"; break;
            case CDE_NO_NAME: why = "an entry without a name"; break;
            case CDE_SEQ_START: why = "a sequence line starting with '>', '@' or '+' (read by the reference)"; rc = PLASSHIP_ERR_UNSUPPORTED; break;
            case CDE_FASTA_MIXED: why = "a line starting with '@' or '+' in a FASTA file (read by the reference)"; rc = PLASSHIP_ERR_UNSUPPORTED; break;
            case CDE_FASTA_CR: why = "a line that holds only '\\r' in a FASTA file (read by the reference)"; rc = PLASSHIP_ERR_UNSUPPORTED; break;
            default: why = "a line of 2^31 bytes or more"; rc = PLASSHIP_ERR_UNSUPPORTED; break;
            }
            setError(std::string(W) + where + why); return rc;
        }
        if (f.fmt == CD_FASTQ && nLines % 4) {
            setError(std::string(W) + f.path + ": not four-line FASTQ (multi-line records, blank lines or a truncated file are read by the reference)"); return PLASSHIP_ERR_UNSUPPORTED;
        }
        if (nRec == 0 || nRec > nLines) { setError(std::string(W) + "internal error (record count)"); return PLASSHIP_ERR_DEVICE; }
        f.nRec = nRec; N += nRec;
        if (N + (uint64_t) P.id_offset >= 0xFFFFFFFFull) { setError(std::string(W) + "too many entries"); return PLASSHIP_ERR_UNSUPPORTED; }
        if (f.recSeqStart.alloc((nRec + 1) * 8) != hipSuccess || f.recName.alloc(nRec * 4) != hipSuccess || f.recHdr.alloc(nRec * 4) != hipSuccess) { setError(std::string(W) + "out of device memory"); return PLASSHIP_ERR_DEVICE; }
        PH_CHECK(kernelsBegin());
        hipLaunchKernelGGL(recordKernel, dim3((unsigned) std::min<uint64_t>((nLines + 255) / 256, grid * 4)), dim3(256), 0, st, f.isHdr.as<uint32_t>(), f.hdrScan.as<uint64_t>(),
                           f.seqPrefix.as<uint64_t>(), hName.as<uint32_t>(), hLen.as<uint32_t>(), nLines, nRec, f.recSeqStart.as<uint64_t>(), f.recName.as<uint32_t>(), f.recHdr.as<uint32_t>());
        if (f.recBase < nSample)
            hipLaunchKernelGGL(probeKernel, dim3(gridRows), dim3(256), 0, st, f.raw.as<unsigned char>(), f.nl.as<uint64_t>(), nLines, f.contrib.as<uint32_t>(), f.hdrScan.as<uint64_t>(),
                               f.recBase, nSample, dProbe.as<unsigned long long>());
        { const int rc = kernelsEnd(msKernel); if (rc) return rc; }      // (hName / hLen go out of scope)
    }
    if (N == 0) { setError(std::string(W) + "the input files have no entry (only FASTA / FASTQ[.gz] is read)"); return PLASSHIP_ERR_IO; }     // createdb.cpp:265-272
    // ---- database type (createdb.cpp:171-200,252): every sampled entry must be > 90 % ACGTUN ----
    if (nSample) {
        unsigned long long pr[20];
        PH_COPY_SYNC(st, pr, dProbe.p, sizeof(pr), hipMemcpyDeviceToHost);
        for (uint64_t g = 0; g < std::min<uint64_t>(N, nSample); g++) {
            const float frac = static_cast<float>(pr[2 * g]) / static_cast<float>(pr[2 * g + 1]);        // 0 / 0 for an empty entry: not > 0.9
            if (!(frac > 0.9)) { setError(std::string(W) + "the input is not a nucleotide read set (entry " + std::to_string(g) + " of the sample is amino acids to the reference's probe); amino-acid input is left to the reference"); return PLASSHIP_ERR_UNSUPPORTED; }
        }
    }
    // ---- placement ----
    KeyMap km; km.splits = P.shuffle ? 32u : 1u; km.idOffset = P.id_offset; km.renumber = P.shuffle ? 1u : 0u;
    { uint32_t run = 0; for (uint32_t s = 0; s < 32; s++) { km.splitBase[s] = run; if (s < km.splits) { const uint64_t i0 = (s + km.splits - km.idOffset % km.splits) % km.splits; run += i0 < N ? (uint32_t) ((N - 1 - i0) / km.splits + 1) : 0u; } } }
    std::unique_ptr<plasship_seqdb> o(new plasship_seqdb()), h(new plasship_seqdb());
    DevBuf seqEnt, hdrEnt, fileK;
    const size_t tmpN = exclusiveScanTmpBytes((size_t) N + 1);
    if (o->d_off.allocLong((N + 2) * 8) != hipSuccess || o->d_len.allocLong((N + 1) * 4) != hipSuccess || o->d_key.allocLong((N + 1) * 4) != hipSuccess ||
        h->d_off.allocLong((N + 2) * 8) != hipSuccess || h->d_len.allocLong((N + 1) * 4) != hipSuccess || h->d_key.allocLong((N + 1) * 4) != hipSuccess ||
        seqEnt.alloc((N + 1) * 4) != hipSuccess || hdrEnt.alloc((N + 1) * 4) != hipSuccess || fileK.alloc((N + 1) * 2) != hipSuccess ||
        (tmpN > dTmp.bytes && dTmp.alloc(tmpN) != hipSuccess)) { setError(std::string(W) + "out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(kernelsBegin());
    for (size_t fi = 0; fi < F.size(); fi++) {
        CdFile &f = *F[fi]; if (!f.nRec) continue;
        ScatterArgs sa; sa.recSeqStart = f.recSeqStart.as<uint64_t>(); sa.recHdr = f.recHdr.as<uint32_t>(); sa.nRec = f.nRec; sa.recBase = f.recBase; sa.fileNo = (uint32_t) fi; sa.km = km;
        sa.seqLenK = o->d_len.as<uint32_t>(); sa.seqEntK = seqEnt.as<uint32_t>(); sa.hdrLenK = h->d_len.as<uint32_t>(); sa.hdrEntK = hdrEnt.as<uint32_t>();
        sa.keyK = o->d_key.as<uint32_t>(); sa.fileK = fileK.as<uint16_t>(); sa.maxLen = dMax.as<unsigned long long>();
        hipLaunchKernelGGL(scatterKernel, dim3((unsigned) std::min<uint64_t>((f.nRec + 255) / 256, grid * 4)), dim3(256), 0, st, sa);
    }
    if (exclusiveScanU32(st, seqEnt.as<uint32_t>(), o->d_off.as<uint64_t>(), N, dTmp.p, dTmp.bytes) ||
        exclusiveScanU32(st, hdrEnt.as<uint32_t>(), h->d_off.as<uint64_t>(), N, dTmp.p, dTmp.bytes)) { setError(std::string(W) + "scan failed"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemcpyAsync(h->d_key.p, o->d_key.p, N * 4, hipMemcpyDeviceToDevice, st));
    uint64_t seqBytes = 0, hdrBytes = 0; unsigned long long mx[2] = {0, 0};
    PH_CHECK(hipMemcpyAsync(&seqBytes, o->d_off.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    PH_CHECK(hipMemcpyAsync(&hdrBytes, h->d_off.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    PH_CHECK(hipMemcpyAsync(mx, dMax.p, 16, hipMemcpyDeviceToHost, st));
    { const int rc = kernelsEnd(msKernel); if (rc) return rc; }
    if (mx[0] > 0x7FFFFFF0ull) { setError(std::string(W) + "a sequence of 2^31 bases or more"); return PLASSHIP_ERR_UNSUPPORTED; }
    if (seqBytes > bytesIn + 2 * N + n_files || hdrBytes > bytesIn + 2 * N + n_files) { setError(std::string(W) + "internal error (output beyond its bound)"); return PLASSHIP_ERR_DEVICE; }
    if (o->d_data.allocLong(seqBytes + 64) != hipSuccess || h->d_data.allocLong(hdrBytes + 64) != hipSuccess) { setError(std::string(W) + "out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync(o->d_data.as<char>() + seqBytes, 0, 64, st)); PH_CHECK(hipMemsetAsync(h->d_data.as<char>() + hdrBytes, 0, 64, st));
    PH_CHECK(kernelsBegin());
    for (size_t fi = 0; fi < F.size(); fi++) {
        CdFile &f = *F[fi]; if (!f.nRec) continue;
        WriteArgs w; w.raw = f.raw.as<unsigned char>(); w.nl = f.nl.as<uint64_t>(); w.nLines = f.nLines; w.isHdr = f.isHdr.as<uint32_t>(); w.contrib = f.contrib.as<uint32_t>();
        w.hdrScan = f.hdrScan.as<uint64_t>(); w.seqPrefix = f.seqPrefix.as<uint64_t>(); w.recSeqStart = f.recSeqStart.as<uint64_t>(); w.recName = f.recName.as<uint32_t>();
        w.recHdr = f.recHdr.as<uint32_t>(); w.recBase = f.recBase; w.km = km; w.seqOff = o->d_off.as<uint64_t>(); w.hdrOff = h->d_off.as<uint64_t>();
        w.seqData = o->d_data.as<unsigned char>(); w.hdrData = h->d_data.as<unsigned char>();
        hipLaunchKernelGGL(writeKernel, dim3((unsigned) std::min<uint64_t>((f.nLines + 15) / 16, (uint64_t) grid * 4)), dim3(256), 0, st, w);
    }
    { const int rc = kernelsEnd(msWrite); if (rc) return rc; }
    msKernel += msWrite;
    F.clear();
    o->dbtype = PLASSHIP_DBTYPE_NUCLEOTIDES; o->n = (size_t) N; o->dataBytes = seqBytes; o->residues = seqBytes - 2 * N; o->maxEntryLen = (uint32_t) mx[0] + 2; o->hostIndexValid = false;
    h->dbtype = 12;             // Parameters::DBTYPE_GENERIC_DB (mm/commons/Parameters.h:77)
    h->n = (size_t) N; h->dataBytes = hdrBytes; h->residues = hdrBytes - 2 * N; h->maxEntryLen = (uint32_t) mx[1] + 2; h->hostIndexValid = false;

    // ---- the stand-alone command's files (createdb.cpp:84,121,291-329) ----
    if (dbPath) {
        const std::string base = dbPath;
        int rc = plasship_seqdb_write(ctx, o.get(), base.c_str()); if (rc) return rc;
        rc = plasship_seqdb_write(ctx, h.get(), (base + "_h").c_str()); if (rc) return rc;
        std::vector<char> hd(hdrBytes + 1); std::vector<uint64_t> ho(N + 1); std::vector<uint16_t> fk(N);
        rc = stagedCopyToHost(ctx, hd.data(), h->d_data.p, hdrBytes); if (rc) return rc;
        rc = stagedCopyToHost(ctx, ho.data(), h->d_off.p, (N + 1) * 8); if (rc) return rc;
        rc = stagedCopyToHost(ctx, fk.data(), fileK.p, N * 2); if (rc) return rc;
        std::string lookup, source, err;
        for (uint64_t k = 0; k < N; k++) {
            const char *p = hd.data() + ho[k]; size_t n = 0;
            while (p[n] && !(p[n] == ' ' || (p[n] >= '\t' && p[n] <= '\r'))) n++;                     // Util::skipNoneWhitespace
            lookup += std::to_string(k); lookup += '\t'; lookup += lookupName(std::string(p, n)); lookup += '\t'; lookup += std::to_string(fk[k]); lookup += '\n';
        }
        for (size_t fi = 0; fi < n_files; fi++) {
            const std::string p = files[fi]; const size_t s = p.find_last_of('/');
            source += std::to_string(fi); source += '\t'; source += s == std::string::npos ? p : p.substr(s + 1); source += '\n';
        }
        if (!writeWholeFile(base + ".lookup", lookup, err) || !writeWholeFile(base + ".source", source, err)) { setError(std::string(W) + err); return PLASSHIP_ERR_IO; }
    }
    if (stats) {
        stats->entries = N; stats->files = n_files; stats->chunks = chunks; stats->bytes_in = bytesIn; stats->bytes_out = seqBytes + hdrBytes; stats->lines = linesAll;
        stats->ms_read = (float) msRead; stats->ms_upload = (float) msUpload; stats->ms_kernel = (float) msKernel; stats->ms_write_kernel = (float) msWrite;
        stats->ms_total = (float) msSinceCd(tAll);
    }
    if (outReads) *outReads = o.release();
    return PLASSHIP_OK;
}

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_createdb(plasship_ctx *ctx, const char *const *files, size_t n_files, const plasship_createdb_params *par,
                                 plasship_seqdb **out_reads, plasship_createdb_stats *stats) {
    if (!out_reads) { setError("plasship_createdb: bad argument (out_reads is NULL)"); return PLASSHIP_ERR_ARG; }
    return createdbImpl(ctx, files, n_files, par, nullptr, out_reads, stats);
}
extern "C" int plasship_createdb_write(plasship_ctx *ctx, const char *const *files, size_t n_files, const plasship_createdb_params *par,
                                       const char *db_path, plasship_seqdb **out_reads, plasship_createdb_stats *stats) {
    if (!db_path) { setError("plasship_createdb_write: bad argument (db_path is NULL)"); return PLASSHIP_ERR_ARG; }
    return createdbImpl(ctx, files, n_files, par, db_path, out_reads, stats);
}
