// What the machine streams, and how close the hash partition of the k-mer records comes to it — development tool.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I plass_amd/csrc tools/linepart_stream_bench.hip -o tools/linepart_stream_bench
//   run:   tools/linepart_stream_bench [records (default 2^30; the 50 M-read step has 3.0-3.9e9)] [timed launches per kernel (default 5)]
// (1) COPY BASELINE: N 16-byte records read once and written once to N slots, consecutive lanes = consecutive records (8 lanes per
//     128-byte line, dwordx4 per lane), persistent workgroups over pieces as linePartKernel has them.  Its best rate is what a
//     kernel that moves these bytes can reach here; the partition's rate is quoted against it, not against the datasheet.
// (2) The two hash-partition launches of kmermatcher (level 1: dense input, value histogram; level 2: line-list input, one piece per
//     level-1 bucket) in the geometry of kmermatch.hip, for every kernel variant listed in VARIANTS, on the same input.
// Every variant's output is checked: per bucket (tag), the number of records and the sum of a hash of each record must equal what the
// input gives for that bucket.  GB/s = (bytes read + bytes written, records only) / time.
#include "linepart.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace plasship;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

typedef Rec<false> R;
typedef void (*PartK)(LinePartArgs);

__device__ __host__ inline uint64_t mix64(uint64_t x) { x += 0x9E3779B97F4A7C15ULL; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 27; x *= 0x94D049BB133111EBULL; x ^= x >> 31; return x; }
__device__ inline uint64_t recHash(const R &r) { return mix64(r.kmer ^ ((uint64_t) r.id << 20) ^ r.len ^ ((uint64_t) (uint16_t) r.pos << 44)); }

__global__ void genKernel(R *out, uint64_t n) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t x = mix64(i);
        R r; r.kmer = (x * 0xD6E8FEB86659FD93ULL) >> 14; r.id = (uint32_t) i; r.len = (uint16_t) (x >> 40); r.pos = (int16_t) (x >> 20);
        out[i] = r;
    }
}

// ---- (1) the copy ----
template <int BLOCK, int ITEMS, bool NT> __global__ __launch_bounds__(BLOCK) void copyKernel(const R *__restrict__ in, R *__restrict__ out, uint64_t n) {
    constexpr uint64_t TILE = (uint64_t) BLOCK * ITEMS;
    for (uint64_t t0 = (uint64_t) blockIdx.x * TILE; t0 < n; t0 += (uint64_t) gridDim.x * TILE) {
        R r[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; u++) { const uint64_t i = t0 + (uint64_t) u * BLOCK + threadIdx.x; if (i < n) r[u] = NT ? streamLoad(in + i) : in[i]; }
#pragma unroll
        for (int u = 0; u < ITEMS; u++) { const uint64_t i = t0 + (uint64_t) u * BLOCK + threadIdx.x; if (i < n) { if (NT) streamStore(out + i, r[u]); else out[i] = r[u]; } }
    }
}

// ---- the check: per tag, records and hash sum (one lane per line; a line's records share the tag) ----
__global__ void sumLinesKernel(const R *__restrict__ recs, const uint32_t *__restrict__ tags, uint64_t nLines, unsigned long long *__restrict__ sums, unsigned long long *__restrict__ counts) {
    for (uint64_t l = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; l < nLines; l += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t t = tags[l];
        if (t == TAG_NONE) continue;
        unsigned long long s = 0, c = 0;
        for (int k = 0; k < RPL; k++) { const R r = recs[l * RPL + k]; if (!isSentinel(r)) { s += recHash(r); c++; } }
        atomicAdd(&sums[t], s); atomicAdd(&counts[t], c);
    }
}
__global__ void sumInputKernel(const R *__restrict__ recs, uint64_t n, int bits, unsigned long long *__restrict__ sums, unsigned long long *__restrict__ counts) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const R r = recs[i];
        const uint32_t t = (uint32_t) (kmerMix<false>(r.kmer) >> (64 - bits));
        atomicAdd(&sums[t], (unsigned long long) recHash(r)); atomicAdd(&counts[t], 1ull);
    }
}

struct Timer {
    hipEvent_t a, b;
    Timer() { CK(hipEventCreate(&a)); CK(hipEventCreate(&b)); }
    template <class F> void run(const char *what, double bytes, int reps, F f) {
        std::vector<float> ms;
        f(); CK(hipDeviceSynchronize());                                              // warm-up
        for (int i = 0; i < reps; i++) { CK(hipEventRecord(a, 0)); f(); CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b)); float t; CK(hipEventElapsedTime(&t, a, b)); ms.push_back(t); }
        CK(hipGetLastError());
        std::sort(ms.begin(), ms.end());
        printf("%-58s min %8.3f  median %8.3f  max %8.3f ms   %7.0f GB/s (median)\n", what, ms.front(), ms[ms.size() / 2], ms.back(), bytes / ms[ms.size() / 2] / 1e6);
        fflush(stdout);
    }
};
static void setLds(PartK k, size_t bytes) { CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes)); }

struct Variant { const char *name; PartK l1, l2; int block; };
#define LP_VARIANT(B, I, D, N) {#B " x " #I " defer=" #D " nt=" #N, linePartKernel<false, false, KEY_HASH, false, true, B, I, true, D, N>, linePartKernel<false, false, KEY_HASH, true, false, B, I, true, D, N>, B}
static const Variant VARIANTS[] = {
    LP_VARIANT(1024, 4, false, false),      // the product's kernel before the deferred store phase
    LP_VARIANT(1024, 4, true, false),
    LP_VARIANT(1024, 4, false, true),
    LP_VARIANT(1024, 4, true, true),
    LP_VARIANT(512, 4, true, true),
    LP_VARIANT(1024, 8, true, true),
    LP_VARIANT(1024, 2, true, true),
};

int main(int argc, char **argv) {
    const uint64_t N = argc > 1 ? strtoull(argv[1], nullptr, 10) : (1ull << 30);
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int numCU = prop.multiProcessorCount;
    printf("device %s, %d CUs; %llu records of %zu bytes = %.2f GB\n", prop.name, numCU, (unsigned long long) N, sizeof(R), N * 16e-9);
    const int b1 = 10, b2 = 10; const uint32_t nb1 = 1u << b1, nb2 = 1u << b2;
    const uint64_t totalLines = (N + RPL - 1) / RPL; const uint32_t lastValid = (uint32_t) (N - (totalLines - 1) * RPL);
    const uint64_t want = (totalLines + 4ull * numCU - 1) / (4ull * numCU);                       // kmermatch.hip: pieceLinesFor, lineGeometry
    const uint32_t PL1 = (uint32_t) std::max<uint64_t>((uint64_t) nb1 * 8, std::min<uint64_t>((uint64_t) nb1 * 64, std::max<uint64_t>(want, 1)));
    const uint64_t nP1 = (totalLines + PL1 - 1) / PL1, cap1 = nP1 * ((uint64_t) PL1 + nb1), cap2 = cap1 + (uint64_t) nb1 * nb2;
    R *dIn, *dL1, *dL2; uint32_t *dTag1, *dTag2, *dList1, *dCnt, *dStart, *dCur, *dNP, *dVH; uint64_t *dRB, *dRE, *dTot; LinePiece *dPieces;
    unsigned long long *dSum, *dNum, *dSumRef, *dNumRef;
    const uint64_t nFine = (uint64_t) nb1 * nb2;
    CK(hipMalloc(&dIn, totalLines * RPL * sizeof(R))); CK(hipMalloc(&dL1, cap1 * RPL * sizeof(R))); CK(hipMalloc(&dL2, cap2 * RPL * sizeof(R)));
    CK(hipMalloc(&dTag1, cap1 * 4)); CK(hipMalloc(&dTag2, cap2 * 4)); CK(hipMalloc(&dList1, cap1 * 4));
    CK(hipMalloc(&dCnt, LP_MAXB * 4)); CK(hipMalloc(&dStart, (LP_MAXB + 1) * 4)); CK(hipMalloc(&dCur, LP_MAXB * 4)); CK(hipMalloc(&dNP, 4)); CK(hipMalloc(&dVH, VH_BINS * 4));
    CK(hipMalloc(&dRB, LP_MAXB * 8)); CK(hipMalloc(&dRE, LP_MAXB * 8)); CK(hipMalloc(&dTot, 8)); CK(hipMalloc(&dPieces, (size_t) nb1 * sizeof(LinePiece)));
    CK(hipMalloc(&dSum, nFine * 8)); CK(hipMalloc(&dNum, nFine * 8)); CK(hipMalloc(&dSumRef, nFine * 8)); CK(hipMalloc(&dNumRef, nFine * 8));
    CK(hipMemset(dIn, 0xFF, totalLines * RPL * sizeof(R)));
    genKernel<<<numCU * 8, 256>>>(dIn, N);
    CK(hipDeviceSynchronize());
    Timer tm;
    const double bytes = 2.0 * N * sizeof(R);

    // ---- (1) ----
    printf("-- copy baseline: read + write of the records, full 128-byte lines\n");
    tm.run("copy 1024 x 4, one workgroup per CU", bytes, reps, [&] { copyKernel<1024, 4, false><<<numCU, 1024>>>(dIn, dL1, N); });
    tm.run("copy 1024 x 4, one workgroup per CU, nontemporal", bytes, reps, [&] { copyKernel<1024, 4, true><<<numCU, 1024>>>(dIn, dL1, N); });
    tm.run("copy 1024 x 4, two workgroups per CU", bytes, reps, [&] { copyKernel<1024, 4, false><<<numCU * 2, 1024>>>(dIn, dL1, N); });
    tm.run("copy 1024 x 4, two workgroups per CU, nontemporal", bytes, reps, [&] { copyKernel<1024, 4, true><<<numCU * 2, 1024>>>(dIn, dL1, N); });
    tm.run("copy 256 x 4, eight workgroups per CU", bytes, reps, [&] { copyKernel<256, 4, false><<<numCU * 8, 256>>>(dIn, dL1, N); });
    tm.run("copy 256 x 4, eight workgroups per CU, nontemporal", bytes, reps, [&] { copyKernel<256, 4, true><<<numCU * 8, 256>>>(dIn, dL1, N); });
    tm.run("copy 256 x 1, eight workgroups per CU, nontemporal", bytes, reps, [&] { copyKernel<256, 1, true><<<numCU * 8, 256>>>(dIn, dL1, N); });
    tm.run("hipMemcpyAsync device to device", bytes, reps, [&] { CK(hipMemcpyAsync(dL1, dIn, N * sizeof(R), hipMemcpyDeviceToDevice, 0)); });

    // ---- (2) ----
    int fails = 0;
    CK(hipMemset(dTag1, 0xFF, cap1 * 4)); CK(hipMemset(dTag2, 0xFF, cap2 * 4));        // lines past the last piece's range: nobody writes them
    std::vector<unsigned long long> refSum[2], refNum[2];
    for (int lvl = 0; lvl < 2; lvl++) {
        const int bits = lvl ? b1 + b2 : b1; const uint64_t nT = 1ull << bits;
        CK(hipMemset(dSumRef, 0, nT * 8)); CK(hipMemset(dNumRef, 0, nT * 8));
        sumInputKernel<<<numCU * 8, 256>>>(dIn, N, bits, dSumRef, dNumRef);
        refSum[lvl].resize(nT); refNum[lvl].resize(nT);
        CK(hipMemcpy(refSum[lvl].data(), dSumRef, nT * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(refNum[lvl].data(), dNumRef, nT * 8, hipMemcpyDeviceToHost));
    }
    auto check = [&](int lvl, const R *recs, const uint32_t *tags, uint64_t cap) {
        const uint64_t nT = refSum[lvl].size();
        CK(hipMemset(dSum, 0, nT * 8)); CK(hipMemset(dNum, 0, nT * 8));
        sumLinesKernel<<<numCU * 8, 256>>>(recs, tags, cap, dSum, dNum);
        std::vector<unsigned long long> s(nT), c(nT);
        CK(hipMemcpy(s.data(), dSum, nT * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(c.data(), dNum, nT * 8, hipMemcpyDeviceToHost));
        uint64_t bad = 0, total = 0;
        for (uint64_t t = 0; t < nT; t++) { if (s[t] != refSum[lvl][t] || c[t] != refNum[lvl][t]) bad++; total += c[t]; }
        printf("    level %d: %llu records in %llu buckets, %llu buckets differ: %s\n", lvl + 1, (unsigned long long) total, (unsigned long long) nT, (unsigned long long) bad, bad || total != N ? "MISMATCH" : "verified");
        if (bad || total != N) fails++;
    };
    const size_t lds1 = linePartLdsBytes(nb1, sizeof(R), true), lds2 = linePartLdsBytes(nb2, sizeof(R), false);
    const unsigned grid1 = (unsigned) std::min<uint64_t>(nP1, (uint64_t) numCU), grid2 = (unsigned) std::min<uint64_t>(nb1, (uint64_t) numCU);
    printf("-- hash partition, 2 x 10 bucket bits, pieces of %u lines at level 1 (%llu pieces), one piece per level-1 bucket at level 2; LDS %zu / %zu bytes\n",
           PL1, (unsigned long long) nP1, lds1, lds2);
    for (const Variant &v : VARIANTS) {
        LinePartArgs a; memset(&a, 0, sizeof(a));
        a.in = dIn; a.out = dL1; a.tags = dTag1; a.totalLines = totalLines; a.lastValidAll = lastValid; a.pieceLines = PL1; a.nb = nb1;
        a.key.shift = 64 - b1; a.valueHist = dVH; a.valueShift = 39;
        setLds(v.l1, lds1); setLds(v.l2, lds2);
        char what[128];
        snprintf(what, sizeof(what), "level 1  %s", v.name);
        tm.run(what, bytes, reps, [&] { hipLaunchKernelGGL(v.l1, dim3(grid1), dim3(v.block), lds1, 0, a); });
        check(0, dL1, dTag1, cap1);
        CK(hipMemset(dCnt, 0, LP_MAXB * 4));
        hipLaunchKernelGGL(tagHistKernel, dim3(numCU * 8), dim3(256), 0, 0, (const uint32_t *) dTag1, cap1, nb1, dCnt);
        hipLaunchKernelGGL(tagScanKernel, dim3(1), dim3(1024), 0, 0, (const uint32_t *) dCnt, nb1, dStart, dCur);
        hipLaunchKernelGGL(tagScatterKernel, dim3(numCU * 2), dim3(TS_BLOCK), 0, 0, (const uint32_t *) dTag1, cap1, nb1, dCur, dList1);
        hipLaunchKernelGGL(planListKernel, dim3(1), dim3(1024), 0, 0, (const uint32_t *) dStart, nb1, 0xFFFFFFFFu, nb2, dPieces, dNP, dRB, dRE, dTot);
        CK(hipDeviceSynchronize());
        LinePartArgs b; memset(&b, 0, sizeof(b));
        b.in = dL1; b.list = dList1; b.out = dL2; b.tags = dTag2; b.pieces = dPieces; b.nPieces = dNP; b.nb = nb2; b.key.shift = 64 - b1 - b2;
        snprintf(what, sizeof(what), "level 2  %s", v.name);
        tm.run(what, bytes, reps, [&] { hipLaunchKernelGGL(v.l2, dim3(grid2), dim3(v.block), lds2, 0, b); });
        check(1, dL2, dTag2, cap2);
    }
    printf("linepart_stream_bench: %d failing checks\n", fails);
    return fails ? 1 : 0;
}
