// The workflows' tail on the device: which contigs are reported, and the FASTA file they go out in.
//   plasship_select_contigs  replaces the `_only_assembled` index filters + createsubdb of data/assemble.sh:170-189 (protein) and
//                            data/nuclassemble.sh:151-169 (nucleotide);
//   plasship_fasta_write     replaces createhdb (src/util/createhdb.cpp:45-58) + convert2fasta (lib/mmseqs/src/util/convert2fasta.cpp:41-56);
//   plasship_subdb_write     replaces createsubdb --subdb-mode 0 and the `_cycle.index` filter of the workflows' --db-mode end
//                            (data/nuclassemble.sh:170-176,200-207; lib/mmseqs/src/util/createsubdb.cpp:41-92).
// "Entry length" is the index length (sequence + "\n\0").  Ranks are key-order ids: the data file of the canonical layout (one file in key
// order: what this library writes, what the reference writes with --threads 1) — the one place where the layout matters is S2 below.
#include "common.hpp"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>
#include <unistd.h>

namespace plasship {

// position of `k` in the ascending array keys[0, n), or -1
__device__ __forceinline__ int64_t findKey(const uint32_t *__restrict__ keys, uint32_t n, uint32_t k) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
    return (lo < n && keys[lo] == k) ? (int64_t) lo : -1;
}
// bytes 1 .. L-2 of a sequence all in 'A'..'Z' (0x41-0x5A), eight at a time: a byte b is outside when (b - 0x41) & 0xFF >= 26
__device__ __forceinline__ bool upperWord(uint64_t w, unsigned nb) {
    bool ok = true;
#pragma unroll
    for (unsigned b = 0; b < 8; b++) { const unsigned c = (unsigned) (w >> (8 * b)) & 0xFFu; ok &= (b >= nb) || (c - 0x41u < 26u); }
    return ok;
}

constexpr uint32_t SEL_S1 = 1u, SEL_S2 = 2u, SEL_WAVE = 4u, SEL_KEEP = 8u;
constexpr uint32_t SHORT_SCAN = 256;     // a "*...*" entry up to this length is scanned by its own thread, a longer one by a wavefront

struct SelArgs {
    SeqView r;                       // RESULT (key order)
    const uint32_t *rKey;
    const uint32_t *sKey, *sLen;     // SOURCE keys (ascending) and sequence lengths
    uint32_t sN;
    int protein, onlyExt;
    int64_t minContigLen;
    uint32_t *flags;                 // [n] SEL_* bits
    uint32_t *keep;                  // [n] 0/1, scanned
    uint32_t *waveList, *waveCount;  // ids whose S2 test needs the wavefront scan
};

// one thread per RESULT entry i (key k, entry length el):
//   S1 / extended: el > the SOURCE entry length of key k (assemble.sh:173-174, nuclassemble.sh:154-155: `$3 > $6` after the key join);
//   S2 (protein):  the entry on data-file line k — id k — is "*[A-Z]*" "*" (assemble.sh:176: the rank of one entry against the key of another;
//                  equal only while the keys are 0..n-1, which --keep-target 0 ends).  First and last byte here, the middle by this thread up to
//                  SHORT_SCAN bytes, else by a wavefront (selWaveKernel);
//   nucleotide:    (mode 0 or extended) and el > --min-contig-len + 1 (nuclassemble.sh:164-167).
__global__ __launch_bounds__(256) void selFlagsKernel(SelArgs a) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < a.r.n; i += gridDim.x * 256) {
        const uint32_t k = a.rKey[i];
        const uint64_t el = (uint64_t) a.r.len[i] + 2;
        const int64_t sp = findKey(a.sKey, a.sN, k);
        const bool ext = sp >= 0 && el > (uint64_t) a.sLen[sp] + 2;
        uint32_t f = ext ? SEL_S1 : 0u;
        bool keep;
        if (a.protein) {
            if (k < a.r.n) {
                const uint32_t L = a.r.len[k];
                const char *p = a.r.data + a.r.off[k];
                if (L >= 2 && p[0] == '*' && p[L - 1] == '*') {
                    if (L <= SHORT_SCAN) {
                        bool ok = true;
                        for (uint32_t j = 1; j + 1 < L; j++) ok &= (unsigned) (unsigned char) p[j] - 0x41u < 26u;
                        if (ok) f |= SEL_S2;
                    } else {
                        f |= SEL_WAVE;
                        a.waveList[atomicAdd(a.waveCount, 1u)] = i;
                    }
                }
            }
            keep = (f & (SEL_S1 | SEL_S2)) != 0;
        } else {
            keep = (!a.onlyExt || ext) && (int64_t) el > a.minContigLen + 1;
        }
        a.flags[i] = f | (keep ? SEL_KEEP : 0u);
        a.keep[i] = keep ? 1u : 0u;
    }
}

// one wavefront per listed id: the middle bytes of the entry on line key[i], 8 bytes per lane and step (a protein contig reaches 65 535 aa)
__global__ __launch_bounds__(256) void selWaveKernel(SelArgs a) {
    const uint32_t nList = *a.waveCount;
    const int lane = laneId();
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nWaves = (gridDim.x * 256) >> 6;
    for (uint32_t w = wave; w < nList; w += nWaves) {
        const uint32_t i = a.waveList[w], k = a.rKey[i];
        const uint32_t L = a.r.len[k];
        const char *p = a.r.data + a.r.off[k] + 1;
        const uint32_t m = L - 2;                      // the middle: bytes 1 .. L-2
        bool ok = true;
        for (uint32_t j = 8u * (uint32_t) lane; j < m; j += 512u) ok &= upperWord(loadU64Unaligned(p + j), min(8u, m - j));   // (buffers are padded past their ends)
        const bool all = __ballot(!ok) == 0ull;
        if (lane == 0 && all) { a.flags[i] |= SEL_S2; a.keep[i] = 1u; }
    }
}

// the subset's index (offsets into the parent's bytes, no copy) and the counts of plasship_select_stats
// stats: [0] selected [1] S1 only [2] S2 only [3] both [4] entry bytes [5] longest entry [6] circular
__global__ __launch_bounds__(256) void selCompactKernel(SeqView r, const uint32_t *__restrict__ rKey, const uint32_t *__restrict__ flags,
                                                        const uint64_t *__restrict__ pos, const uint32_t *__restrict__ cKey, uint32_t cN,
                                                        uint64_t *__restrict__ oOff, uint32_t *__restrict__ oLen, uint32_t *__restrict__ oKey,
                                                        unsigned long long *__restrict__ stats) {
    unsigned long long c1 = 0, c2 = 0, c12 = 0, bytes = 0, mx = 0, cyc = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < r.n; i += gridDim.x * 256) {
        const uint32_t f = flags[i];
        const bool keep = (f & SEL_KEEP) || (f & SEL_S2);          // (a wavefront-tested S2 entry was marked after selFlagsKernel)
        if (!keep) continue;
        const uint64_t j = pos[i];
        const uint32_t L = r.len[i], k = rKey[i];
        oOff[j] = r.off[i]; oLen[j] = L; oKey[j] = k;
        const bool s1 = f & SEL_S1, s2 = f & SEL_S2;
        c1 += s1 && !s2; c2 += s2 && !s1; c12 += s1 && s2;
        bytes += (uint64_t) L + 2; mx = max(mx, (unsigned long long) L + 2);
        if (cKey && findKey(cKey, cN, k) >= 0) cyc++;
    }
    c1 = waveReduceSumU64(c1); c2 = waveReduceSumU64(c2); c12 = waveReduceSumU64(c12); bytes = waveReduceSumU64(bytes); cyc = waveReduceSumU64(cyc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(mx, o, 64); mx = t > mx ? t : mx; }
    if (laneId() == 0) {
        if (c1) atomicAdd(&stats[1], c1);
        if (c2) atomicAdd(&stats[2], c2);
        if (c12) atomicAdd(&stats[3], c12);
        if (bytes) atomicAdd(&stats[4], bytes);
        if (mx) atomicMax(&stats[5], mx);
        if (cyc) atomicAdd(&stats[6], cyc);
    }
}

// ---- FASTA ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t decDigits(uint64_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; d++; } return d; }
// ">" rank " len:" L [" cycle:" c] "\n" — the header line of createhdb.cpp:50-58 as convert2fasta.cpp:47-49 writes it
__device__ __forceinline__ uint32_t headerBytes(uint64_t rank, uint32_t L, bool hasCycle) { return 1 + decDigits(rank) + 5 + decDigits(L) + (hasCycle ? 8 : 0) + 1; }

// per entry: output bytes (header + sequence + "\n") and, with a cycle DB, whether its key is in it
__global__ __launch_bounds__(256) void fastaSizeKernel(const uint32_t *__restrict__ len, const uint32_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ cKey,
                                                       uint32_t cN, int hasCycle, uint64_t *__restrict__ size, unsigned char *__restrict__ cyc) {
    for (uint64_t r = (uint64_t) blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t) gridDim.x * 256) {
        const uint32_t L = len[r];
        size[r] = headerBytes(r, L, hasCycle) + (uint64_t) L + 1;
        if (hasCycle) cyc[r] = (cKey && findKey(cKey, cN, key[r]) >= 0) ? 1 : 0;
    }
}
// first entry of every output chunk of `chunkBytes` (by the output offset where the entry starts); bound[nChunks] = n
__global__ void fastaChunkKernel(const uint64_t *__restrict__ outOff, uint64_t n, uint64_t chunkBytes, uint64_t nChunks, uint64_t *__restrict__ bound) {
    for (uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c <= nChunks; c += (uint64_t) gridDim.x * blockDim.x) {
        if (c == nChunks) { bound[c] = n; continue; }
        uint64_t lo = 0, hi = n;                       // first r with outOff[r] >= c * chunkBytes
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (outOff[mid] < c * chunkBytes) lo = mid + 1; else hi = mid; }
        bound[c] = lo;
    }
}
// entries [b, e) into `out` (byte 0 = the first byte of entry b).  Every lane formats its own entry's header; then the wavefront copies the
// sequences of its 64 entries one after the other with all 64 lanes, 8 bytes per lane and step (the copy of appendOutKernel, outdb.hip)
__global__ __launch_bounds__(256) void fastaWriteKernel(const char *data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                        const uint64_t *__restrict__ outOff, const unsigned char *__restrict__ cyc, int hasCycle,
                                                        uint64_t b, uint64_t e, char *__restrict__ out) {
    const int lane = laneId();
    const uint64_t base = outOff[b];
    for (uint64_t r0 = b + (uint64_t) blockIdx.x * 256 + (threadIdx.x & ~63u); r0 < e; r0 += (uint64_t) gridDim.x * 256) {
        const uint64_t r = r0 + (uint64_t) lane;
        uint32_t L = 0; uint64_t src = 0, dst = 0;
        if (r < e) {
            L = len[r]; src = off[r];
            char *h = out + (outOff[r] - base);
            uint32_t p = 0;
            h[p++] = '>';
            const uint32_t dr = decDigits(r);
            { uint64_t v = r; for (uint32_t d = dr; d > 0; d--) { h[p + d - 1] = (char) ('0' + v % 10); v /= 10; } p += dr; }
            h[p++] = ' '; h[p++] = 'l'; h[p++] = 'e'; h[p++] = 'n'; h[p++] = ':';
            const uint32_t dl = decDigits(L);
            { uint32_t v = L; for (uint32_t d = dl; d > 0; d--) { h[p + d - 1] = (char) ('0' + v % 10); v /= 10; } p += dl; }
            if (hasCycle) { const char *cs = " cycle:"; for (int q = 0; q < 7; q++) h[p++] = cs[q]; h[p++] = cyc[r] ? '1' : '0'; }
            h[p++] = '\n';
            dst = (outOff[r] - base) + p;
            out[dst + L] = '\n';
        }
        unsigned long long m = __ballot(L != 0);
        while (m) {
            const int s = __ffsll((long long) m) - 1;
            m &= m - 1;
            const uint32_t cl = (uint32_t) __shfl((int) L, s, 64);
            const uint64_t cs = (uint64_t) __shfl((unsigned long long) src, s, 64), cd = (uint64_t) __shfl((unsigned long long) dst, s, 64);
            const char *from = data + cs; char *to = out + cd;
            for (uint32_t q = 8u * (uint32_t) lane; q < cl; q += 512u) {
                const uint64_t x = loadU64Unaligned(from + q);                         // (sequence buffers are padded past their ends)
                if (q + 8 <= cl) storeU64Unaligned(to + q, x); else storeTail(to + q, x, cl - q);
            }
        }
    }
}

// ---- createsubdb --subdb-mode 0 ---------------------------------------------------------------------------------------------------
// A subset made by plasship_select_contigs is an index over its parent's bytes; the DB createsubdb writes holds the listed entries back to
// back in list order (createsubdb.cpp:66-79).  Entry bytes ("SEQ\n\0") per entry, a prefix sum, then one wavefront per entry.
__global__ __launch_bounds__(256) void subdbBytesKernel(const uint32_t *__restrict__ len, uint64_t n, uint64_t *__restrict__ bytes) {
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t) gridDim.x * 256) bytes[i] = (uint64_t) len[i] + 2;
}
// 16 bytes per lane and step.  Neither end of the copy is aligned (entries start anywhere in both buffers): the bytes go through
// __builtin_memcpy, whose alignment of 1 lets the compiler pick what the target allows — global memory takes unaligned dwordx4 accesses on
// gfx950, so this is one load and one store per lane and step.  The last 1-15 bytes of an entry are copied byte by byte: nothing is read or
// written beyond the entry, so the kernel does not lean on the padding behind the buffers.
__global__ __launch_bounds__(256) void subdbGatherKernel(const char *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                         const uint64_t *__restrict__ newOff, uint64_t n, char *__restrict__ out) {
    const uint32_t lane = (uint32_t) laneId();
    const uint64_t wave = ((uint64_t) blockIdx.x * 256 + threadIdx.x) >> 6, nWaves = ((uint64_t) gridDim.x * 256) >> 6;
    for (uint64_t i = wave; i < n; i += nWaves) {
        const uint32_t el = len[i] + 2;
        const char *from = data + off[i];
        char *to = out + newOff[i];
        for (uint32_t q = 16u * lane; q < el; q += 1024u) {
            if (q + 16u <= el) { uint4 x; __builtin_memcpy(&x, from + q, 16); __builtin_memcpy(to + q, &x, 16); }
            else for (uint32_t b = q; b < el; b++) to[b] = from[b];
        }
    }
}

static unsigned gridFor(uint64_t n, int numCU) { return (unsigned) std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t) numCU * 16)); }

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_select_contigs(plasship_ctx *ctx, const plasship_seqdb *result, const plasship_seqdb *source, const plasship_seqdb *cycles,
                                       const plasship_select_params *par, plasship_seqdb **out, plasship_select_stats *stats) {
    if (!ctx || !result || !source || !par || !out) { setError("plasship_select_contigs: bad argument"); return PLASSHIP_ERR_ARG; }
    if (par->mode != PLASSHIP_SELECT_PROTEIN && par->mode != PLASSHIP_SELECT_NUCLEOTIDE) { setError("plasship_select_contigs: mode must be PLASSHIP_SELECT_PROTEIN or _NUCLEOTIDE"); return PLASSHIP_ERR_ARG; }
    if (par->min_contig_len < 0) { setError("plasship_select_contigs: min_contig_len must not be negative"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const uint32_t N = (uint32_t) result->n;
    PH_CHECK(hipEventRecord(ctx->ev[0], st));
    DevBuf dFlags, dKeep, dPos, dList, dStats, dTmp;
    const size_t tmpBytes = exclusiveScanTmpBytes((size_t) N + 2);
    if (dFlags.alloc(((size_t) N + 1) * 4) != hipSuccess || dKeep.alloc(((size_t) N + 1) * 4) != hipSuccess || dPos.alloc(((size_t) N + 2) * 8) != hipSuccess ||
        dList.alloc(((size_t) N + 1) * 4) != hipSuccess || dStats.alloc(8 * 8) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess) {
        setError("plasship_select_contigs: out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 8 * 8, st));
    SelArgs a;
    a.r = result->view(); a.rKey = result->d_key.as<uint32_t>();
    a.sKey = source->d_key.as<uint32_t>(); a.sLen = source->d_len.as<uint32_t>(); a.sN = (uint32_t) source->n;
    a.protein = par->mode == PLASSHIP_SELECT_PROTEIN; a.onlyExt = par->only_extended != 0; a.minContigLen = par->min_contig_len;
    a.flags = dFlags.as<uint32_t>(); a.keep = dKeep.as<uint32_t>(); a.waveList = dList.as<uint32_t>(); a.waveCount = dStats.as<uint32_t>() + 14;   // (the last word of dStats)
    if (N) {
        hipLaunchKernelGGL(selFlagsKernel, dim3(gridFor(N, ctx->numCU)), dim3(256), 0, st, a);
        if (a.protein) hipLaunchKernelGGL(selWaveKernel, dim3((unsigned) ctx->numCU * 8), dim3(256), 0, st, a);
    }
    if (exclusiveScanU32(st, dKeep.as<uint32_t>(), dPos.as<uint64_t>(), N, dTmp.p, tmpBytes)) { setError("plasship_select_contigs: scan failed"); return PLASSHIP_ERR_DEVICE; }
    uint64_t M = 0;
    PH_COPY_SYNC(st, &M, dPos.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost);
    std::unique_ptr<plasship_seqdb> o(new plasship_seqdb());
    if (o->d_off.allocLong((M + 1) * 8) != hipSuccess || o->d_len.allocLong((M + 1) * 4) != hipSuccess || o->d_key.allocLong((M + 1) * 4) != hipSuccess) {
        setError("plasship_select_contigs: out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    if (N) hipLaunchKernelGGL(selCompactKernel, dim3(gridFor(N, ctx->numCU)), dim3(256), 0, st, a.r, a.rKey, (const uint32_t *) dFlags.as<uint32_t>(),
                              (const uint64_t *) dPos.as<uint64_t>(), cycles ? (const uint32_t *) cycles->d_key.as<uint32_t>() : nullptr, cycles ? (uint32_t) cycles->n : 0u,
                              o->d_off.as<uint64_t>(), o->d_len.as<uint32_t>(), o->d_key.as<uint32_t>(), dStats.as<unsigned long long>());
    PH_CHECK(hipEventRecord(ctx->ev[1], st));
    unsigned long long s[7] = {0, 0, 0, 0, 0, 0, 0};
    PH_COPY_SYNC(st, s, dStats.p, sizeof(s), hipMemcpyDeviceToHost);
    float ms = 0; PH_CHECK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    // the subset is an index over its parent's bytes: it shares the parent's heap, or borrows the parent's buffer
    o->dbtype = result->dbtype; o->n = (size_t) M;
    o->heap = result->heap;
    if (!o->heap) o->borrowedData = result->dataPtr();
    o->contiguous = result->contiguous && M == result->n;
    o->dataBytes = s[4]; o->residues = s[4] - 2 * M; o->maxEntryLen = (uint32_t) s[5];
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->n_selected = M; stats->n_s1_only = s[1]; stats->n_s2_only = s[2]; stats->n_both = s[3]; stats->n_cycle = s[6]; stats->ms_kernel = ms;
    }
    *out = o.release();
    return PLASSHIP_OK;
}

extern "C" int plasship_fasta_write(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_seqdb *cycles, const char *path, plasship_fasta_stats *stats) {
    if (!ctx || !db || !path) { setError("plasship_fasta_write: bad argument"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const uint64_t n = db->n;
    const int hasCycle = cycles != nullptr;
    const double t0 = ioNow();
    PH_CHECK(hipEventRecord(ctx->ev[0], st));
    DevBuf dOut, dCyc, dBound, dTmp, dBuf[2];
    const size_t tmpBytes = exclusiveScanTmpBytes((size_t) n + 2);
    if (dOut.alloc((n + 2) * 8) != hipSuccess || dCyc.alloc(n + 1) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess) { setError("plasship_fasta_write: out of device memory"); return PLASSHIP_ERR_DEVICE; }
    if (n) hipLaunchKernelGGL(fastaSizeKernel, dim3(gridFor(n, ctx->numCU)), dim3(256), 0, st, (const uint32_t *) db->d_len.as<uint32_t>(), (const uint32_t *) db->d_key.as<uint32_t>(), n,
                              hasCycle ? (const uint32_t *) cycles->d_key.as<uint32_t>() : nullptr, hasCycle ? (uint32_t) cycles->n : 0u, hasCycle, dOut.as<uint64_t>(), dCyc.as<unsigned char>());
    if (exclusiveScanU64(st, dOut.as<uint64_t>(), dOut.as<uint64_t>(), n, dTmp.p, tmpBytes)) { setError("plasship_fasta_write: scan failed"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipEventRecord(ctx->ev[1], st));
    uint64_t total = 0;
    PH_COPY_SYNC(st, &total, dOut.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost);
    float msKernel0 = 0; PH_CHECK(hipEventElapsedTime(&msKernel0, ctx->ev[0], ctx->ev[1]));
    // chunks of about chunkBytes of output (entries whole: a chunk ends where an entry starting past its end begins), formatted into one
    // of two device buffers: the next chunk is formatted ahead of the copy of this one, which streams to the file through the pinned
    // staging buffers while the previous part is written (stagedDownload)
    const uint64_t chunkBytes = (uint64_t) std::max(1, tuneInt("FASTA_CHUNK_MB", 256)) << 20;
    const uint64_t nChunks = n ? (total + chunkBytes - 1) / chunkBytes : 0;
    std::vector<uint64_t> bound(nChunks + 1, 0), outOffAt(nChunks + 1, 0);
    const uint64_t maxEntryOut = (uint64_t) db->maxEntryLen + 64;
    const uint64_t bufBytes = std::min<uint64_t>(total, chunkBytes + maxEntryOut) + 64;
    if (nChunks) {
        if (dBound.alloc((nChunks + 1) * 8) != hipSuccess || dBuf[0].alloc(bufBytes) != hipSuccess || (nChunks > 1 && dBuf[1].alloc(bufBytes) != hipSuccess)) {
            setError("plasship_fasta_write: out of device memory"); return PLASSHIP_ERR_DEVICE;
        }
        hipLaunchKernelGGL(fastaChunkKernel, dim3((unsigned) std::min<uint64_t>((nChunks + 256) / 256, 1024)), dim3(256), 0, st, (const uint64_t *) dOut.as<uint64_t>(), n, chunkBytes, nChunks, dBound.as<uint64_t>());
        PH_COPY_SYNC(st, bound.data(), dBound.p, (nChunks + 1) * 8, hipMemcpyDeviceToHost);
    }
    // output offset where each chunk starts (host copy of outOff at the bounds)
    for (uint64_t c = 0; c <= nChunks; c++) {
        if (bound[c] >= n) { outOffAt[c] = total; continue; }
        PH_COPY_SYNC(st, &outOffAt[c], dOut.as<uint64_t>() + bound[c], 8, hipMemcpyDeviceToHost);
    }
    for (uint64_t c = 0; c < nChunks; c++)
        if (outOffAt[c + 1] - outOffAt[c] + 64 > bufBytes) { setError("plasship_fasta_write: chunk larger than its buffer"); return PLASSHIP_ERR_DEVICE; }
    // kernel time: the size pass and every chunk's formatting, each between two events of its own (ev[2..5]: two chunks in flight)
    float msKernel = 0;
    auto format = [&](uint64_t c) -> int {
        const uint64_t b = bound[c], e = bound[c + 1];
        PH_CHECK(hipEventRecord(ctx->ev[2 + 2 * (c & 1)], st));
        if (e > b) hipLaunchKernelGGL(fastaWriteKernel, dim3(gridFor(e - b, ctx->numCU)), dim3(256), 0, st, db->dataPtr(), (const uint64_t *) db->d_off.as<uint64_t>(),
                                      (const uint32_t *) db->d_len.as<uint32_t>(), (const uint64_t *) dOut.as<uint64_t>(), (const unsigned char *) dCyc.as<unsigned char>(), hasCycle,
                                      b, e, dBuf[c & 1].as<char>());
        PH_CHECK(hipEventRecord(ctx->ev[3 + 2 * (c & 1)], st));
        return PLASSHIP_OK;
    };
    auto formatTime = [&](uint64_t c) -> int {       // (after the copy of chunk c: its formatting has long completed)
        float t = 0; PH_CHECK(hipEventElapsedTime(&t, ctx->ev[2 + 2 * (c & 1)], ctx->ev[3 + 2 * (c & 1)])); msKernel += t;
        return PLASSHIP_OK;
    };
    // "<path>.tmp.<pid>", renamed into place when everything is written (the convention of DBFileWriter, host_util.hpp)
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long) getpid());
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp) { setError(std::string("plasship_fasta_write: cannot open ") + tmp + ": " + strerror(errno)); return PLASSHIP_ERR_IO; }
    bool failed = false; int rc = PLASSHIP_OK;
    if (nChunks) rc = format(0);
    for (uint64_t c = 0; c < nChunks && !rc; c++) {
        if (c + 1 < nChunks && (rc = format(c + 1)) != PLASSHIP_OK) break;
        rc = stagedDownload(ctx, dBuf[c & 1].p, outOffAt[c + 1] - outOffAt[c], [&](const char *src, uint64_t, uint64_t nb) {
            if (fwrite(src, 1, (size_t) nb, fp) != (size_t) nb) failed = true;
            return !failed;
        });
        if (!rc) { PH_CHECK(plasship::streamSync(st)); rc = formatTime(c); }
    }
    if (fclose(fp) != 0) failed = true;
    if (rc || failed) { unlink(tmp.c_str()); setError(std::string("plasship_fasta_write: error while writing ") + path); return rc ? rc : PLASSHIP_ERR_IO; }
    if (rename(tmp.c_str(), path) != 0) { unlink(tmp.c_str()); setError(std::string("plasship_fasta_write: cannot rename ") + tmp + " to " + path); return PLASSHIP_ERR_IO; }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->n_entries = n; stats->bytes = total; stats->n_chunks = nChunks; stats->ms_kernel = msKernel0 + msKernel; stats->ms_total = (float) ((ioNow() - t0) * 1e3);
    }
    return PLASSHIP_OK;
}

extern "C" int plasship_subdb_write(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_seqdb *cycles, const char *path, plasship_subdb_stats *stats) {
    if (!ctx || !db || !path) { setError("plasship_subdb_write: bad argument"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const uint64_t n = db->n;
    const double t0 = ioNow();
    PH_CHECK(hipEventRecord(ctx->ev[0], st));
    DevBuf dOff, dTmp, dOut;
    const size_t tmpBytes = exclusiveScanTmpBytes((size_t) n + 2);
    if (dOff.alloc((n + 2) * 8) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess) { setError("plasship_subdb_write: out of device memory"); return PLASSHIP_ERR_DEVICE; }
    if (n) hipLaunchKernelGGL(subdbBytesKernel, dim3(gridFor(n, ctx->numCU)), dim3(256), 0, st, (const uint32_t *) db->d_len.as<uint32_t>(), n, dOff.as<uint64_t>());
    if (exclusiveScanU64(st, dOff.as<uint64_t>(), dOff.as<uint64_t>(), n, dTmp.p, tmpBytes)) { setError("plasship_subdb_write: scan failed"); return PLASSHIP_ERR_DEVICE; }
    uint64_t total = 0;
    PH_COPY_SYNC(st, &total, dOff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost);
    if (dOut.alloc(total + 64) != hipSuccess) { setError("plasship_subdb_write: out of device memory"); return PLASSHIP_ERR_DEVICE; }
    // one wavefront per entry, four to a block
    if (n) hipLaunchKernelGGL(subdbGatherKernel, dim3((unsigned) std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t) ctx->numCU * 16))), dim3(256), 0, st, db->dataPtr(),
                              (const uint64_t *) db->d_off.as<uint64_t>(), (const uint32_t *) db->d_len.as<uint32_t>(), (const uint64_t *) dOff.as<uint64_t>(), n, dOut.as<char>());
    PH_CHECK(hipEventRecord(ctx->ev[1], st));
    PH_CHECK(plasship::streamSync(st));
    PH_CHECK(hipGetLastError());
    float ms = 0; PH_CHECK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    // the index: keys and entry lengths in list order (a handle's order is key order, so the list is ordered and createsubdb leaves the
    // index as written: createsubdb.cpp:57-58,88)
    std::vector<uint32_t> key(n), elen(n), cyc;
    if (n) {
        int rc = stagedCopyToHost(ctx, key.data(), db->d_key.p, n * 4); if (rc) return rc;
        rc = stagedCopyToHost(ctx, elen.data(), db->d_len.p, n * 4); if (rc) return rc;
        for (uint64_t i = 0; i < n; i++) elen[i] += 2;
    }
    if (cycles && cycles->n) { cyc.resize(cycles->n); const int rc = stagedCopyToHost(ctx, cyc.data(), cycles->d_key.p, cycles->n * 4); if (rc) return rc; }
    std::string err; DBFileWriter w;
    if (!w.open(path, db->dbtype, err)) { setError(err); return PLASSHIP_ERR_IO; }
    if (total) {
        const int rc = stagedDownload(ctx, dOut.p, total, [&](const char *src, uint64_t, uint64_t nb) { w.data(src, (size_t) nb); return !w.failed; });
        if (rc == PLASSHIP_ERR_IO) setError(std::string("error while writing ") + path);
        if (rc) return rc;
    }
    w.index(key.data(), elen.data(), (size_t) n);
    if (!w.close(err)) { setError(err); return PLASSHIP_ERR_IO; }
    // "<path>_cycle.index": the lines of the index just written whose key is circular (nuclassemble.sh:173-175,204-206); the file exists
    // whenever a cycle DB does, with or without lines
    uint64_t nCyc = 0;
    if (cycles) {
        std::string text; char tmp[80]; uint64_t o = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (std::binary_search(cyc.begin(), cyc.end(), key[i])) {          // (a handle's keys are ascending)
                char *q = fmtU32(key[i], tmp); *q++ = '\t'; q = fmtU64(o, q); *q++ = '\t'; q = fmtU64(elen[i], q); *q++ = '\n';
                text.append(tmp, (size_t) (q - tmp)); nCyc++;
            }
            o += elen[i];
        }
        const std::string name = std::string(path) + "_cycle.index", tmpName = name + ".tmp." + std::to_string((long) getpid());
        FILE *fp = fopen(tmpName.c_str(), "wb");
        bool ok = fp != nullptr;
        if (fp) { ok = fwrite(text.data(), 1, text.size(), fp) == text.size(); ok &= fclose(fp) == 0; }
        if (ok) ok = rename(tmpName.c_str(), name.c_str()) == 0;
        if (!ok) { unlink(tmpName.c_str()); setError("plasship_subdb_write: cannot write " + name); return PLASSHIP_ERR_IO; }
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->n_entries = n; stats->bytes = total; stats->n_cycle = nCyc; stats->ms_kernel = ms; stats->ms_total = (float) ((ioNow() - t0) * 1e3);
    }
    return PLASSHIP_OK;
}
