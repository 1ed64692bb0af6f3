// The line lists of the hash partition against a plain copy of the same bytes — development tool, the method of linepart_stream_bench.hip.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I plass_amd/csrc tools/linelist_bench.hip -o tools/linelist_bench
//   run:   tools/linelist_bench [tags (default 430000000)] [timed launches per kernel (default 5)] [key set (default all)] [current]
//          ("current": only the three kernels of the parent commit, for counter passes)
// Tag arrays in the shape of the 50 M-read step: level 1 = pieces of 65 536 + 1024 output lines, 1024 buckets, the lines a piece did not
// use tagged TAG_NONE at its end; level 2 = 1024 regions (one per level-1 bucket) of 1024 fine buckets, TAG_NONE at every region's end.
// Key sets: uniform, skewed (the square of a uniform variable: a quarter of the lines in 1/16 of the buckets), equal (all lines in one
// bucket), hole (uniform, one bucket without a line).  Timed: tagHistKernel, tagScatterKernel and tagSortRegionKernel as the parent commit
// launches them, every run-list variant, and a copy that reads the tags and writes as many list entries.  Every variant is checked on the
// device: the list range of bucket b (start[b] .. start[b + 1], resp. fineBeg / fineCnt) must hold line numbers whose tag is b, no line
// twice, and the ranges together as many entries as there are tagged lines.  ratio = median time / median time of the best copy.
#include "linepart.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace plasship;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

__device__ __host__ inline uint64_t mix64(uint64_t x) { x += 0x9E3779B97F4A7C15ULL; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 27; x *= 0x94D049BB133111EBULL; x ^= x >> 31; return x; }
enum { KS_UNIFORM = 0, KS_SKEWED = 1, KS_EQUAL = 2, KS_HOLE = 3 };
static const char *const KS_NAME[4] = {"uniform", "skewed", "equal", "hole"};
__device__ inline uint32_t keyBucket(int ks, uint64_t i, uint32_t nb) {
    const uint32_t u = (uint32_t) (mix64(i) >> 40) & 0xFFFFu;                    // 16 uniform bits
    uint32_t b = ks == KS_SKEWED ? (uint32_t) (((uint64_t) u * u) >> 16) * nb >> 16 : ks == KS_EQUAL ? 7u % nb : (u * nb) >> 16;
    if (ks == KS_HOLE && b == 5) b = 6;
    return b;
}
// span s (a level-1 piece, a level-2 region) = lines [beg[s], end[s]); its first `used` = len - tail lines carry tags, the rest TAG_NONE
__global__ void genTagsKernel(uint32_t *tags, const uint64_t *__restrict__ beg, const uint64_t *__restrict__ end, uint32_t nSpans, uint32_t tail, int ks, uint32_t nb, int perSpanBase) {
    for (uint32_t s = blockIdx.x; s < nSpans; s += gridDim.x) {
        const uint64_t b0 = beg[s], len = end[s] - b0, used = len > tail ? len - tail : 0;
        for (uint64_t j = threadIdx.x; j < len; j += blockDim.x) tags[b0 + j] = j < used ? (perSpanBase ? s * nb : 0u) + keyBucket(ks, b0 + j, nb) : TAG_NONE;
    }
}
template <bool V4> __global__ __launch_bounds__(1024) void copyTagsKernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint64_t n) {
    if (V4) { for (uint64_t i = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) * 4; i + 4 <= n; i += (uint64_t) gridDim.x * blockDim.x * 4) *reinterpret_cast<uint4 *>(out + i) = *reinterpret_cast<const uint4 *>(in + i); }
    else for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) out[i] = in[i];
}
__global__ void countTaggedKernel(const uint32_t *__restrict__ tags, uint64_t n, unsigned long long *out) {
    unsigned long long c = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) c += tags[i] != TAG_NONE;
    c = waveReduceSumU64(c);
    if (laneId() == 0 && c) atomicAdd(out, c);
}
// one workgroup per bucket and round: res[0] += entries that name a line of the bucket for the first time, res[1] += all others
__global__ void checkListKernel(const uint32_t *__restrict__ tags, uint64_t nLines, const uint32_t *__restrict__ list, const uint32_t *__restrict__ beg, const uint32_t *__restrict__ cnt,
                                const uint32_t *__restrict__ start, uint32_t nBuckets, uint32_t *seen, unsigned long long *res) {
    unsigned long long good = 0, bad = 0;
    for (uint32_t b = blockIdx.x; b < nBuckets; b += gridDim.x) {
        const uint32_t p0 = start ? start[b] : beg[b], c = start ? start[b + 1] - p0 : cnt[b];
        for (uint32_t j = threadIdx.x; j < c; j += blockDim.x) {
            const uint64_t p = (uint64_t) p0 + j;
            bool ok = p < nLines;
            if (ok) { const uint32_t e = list[p]; ok = e < nLines && tags[e] == b && !((atomicOr(&seen[e >> 5], 1u << (e & 31)) >> (e & 31)) & 1u); }
            if (ok) good++; else bad++;
        }
    }
    good = waveReduceSumU64(good); bad = waveReduceSumU64(bad);
    if (laneId() == 0) { if (good) atomicAdd(&res[0], good); if (bad) atomicAdd(&res[1], bad); }
}

struct Timer {
    hipEvent_t a, b; double copyMs = 0;
    Timer() { CK(hipEventCreate(&a)); CK(hipEventCreate(&b)); }
    template <class F> double run(const char *what, double bytes, int reps, F f) {
        std::vector<float> ms;
        f(); CK(hipDeviceSynchronize());                                              // warm-up
        for (int i = 0; i < reps; i++) { CK(hipEventRecord(a, 0)); f(); CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b)); float t; CK(hipEventElapsedTime(&t, a, b)); ms.push_back(t); }
        CK(hipGetLastError());
        std::sort(ms.begin(), ms.end());
        const double med = ms[ms.size() / 2];
        printf("  %-64s min %7.3f  median %7.3f  max %7.3f ms  %6.0f GB/s", what, ms.front(), med, ms.back(), bytes / med / 1e6);
        if (copyMs > 0) printf("  %5.2f x copy", med / copyMs);
        printf("\n"); fflush(stdout);
        return med;
    }
};
typedef void (*ScatterK)(const uint32_t *, uint64_t, uint32_t, uint32_t *, uint32_t *);
typedef void (*RegionK)(const uint32_t *, const uint64_t *, const uint64_t *, uint32_t, uint32_t, uint32_t *, uint32_t *, uint32_t *);
struct ScatterV { const char *name; ScatterK k; int block, chunk; };
struct RegionV { const char *name; RegionK k; int block, chunk; };
#define SV(B, C) {"tagScatterRunsKernel<" #B ", " #C ">", tagScatterRunsKernel<B, C>, B, C}
#define RV(B, C) {"tagSortRegionRunsKernel<" #B ", " #C ">", tagSortRegionRunsKernel<B, C>, B, C}
static const ScatterV SCATTER[] = {SV(1024, 32768), SV(1024, 16384), SV(512, 16384), SV(512, 8192), SV(1024, 8192)};
static const RegionV REGION[] = {RV(1024, 32768), RV(1024, 16384), RV(512, 16384), RV(512, 8192), RV(1024, 8192)};
static unsigned perCU(size_t lds, int block) { return (unsigned) std::max<size_t>(1, std::min<size_t>(2048 / block, (160 * 1024) / (lds + 1024))); }

int main(int argc, char **argv) {
    const uint64_t want = argc > 1 ? strtoull(argv[1], nullptr, 10) : 430000000ull;
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    const std::string only = argc > 3 ? argv[3] : "all";
    const bool currentOnly = argc > 4 && !strcmp(argv[4], "current");
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int numCU = prop.multiProcessorCount;
    const uint32_t nb1 = 1024, nb2 = 1024, PL = 65536, pieceOut = PL + nb1;
    const uint32_t nP = (uint32_t) std::max<uint64_t>(1, want / pieceOut);
    const uint64_t cap1 = (uint64_t) nP * pieceOut, regLen = cap1 / nb1 + nb2, cap2 = regLen * nb1;
    if (cap2 >= 0xFFFFFFFFull) { fprintf(stderr, "too many tags\n"); return 2; }
    printf("device %s, %d CUs; level 1: %u pieces of %u lines = %llu tags (%.2f GB); level 2: %u regions of %llu lines = %llu tags\n", prop.name, numCU, nP, pieceOut,
           (unsigned long long) cap1, cap1 * 4e-9, nb1, (unsigned long long) regLen, (unsigned long long) cap2);
    std::vector<uint64_t> pb(nP), pe(nP), rb(nb1), re(nb1);
    for (uint32_t p = 0; p < nP; p++) { pb[p] = (uint64_t) p * pieceOut; pe[p] = pb[p] + pieceOut; }
    for (uint32_t g = 0; g < nb1; g++) { rb[g] = (uint64_t) g * regLen; re[g] = rb[g] + regLen; }
    uint32_t *dTag1, *dTag2, *dList, *dCnt, *dStart, *dCur, *dFBeg, *dFCnt, *dSeen; uint64_t *dPB, *dPE, *dRB, *dRE; unsigned long long *dRes;
    CK(hipMalloc(&dTag1, cap1 * 4)); CK(hipMalloc(&dTag2, cap2 * 4)); CK(hipMalloc(&dList, cap2 * 4)); CK(hipMalloc(&dSeen, (cap2 / 32 + 1) * 4));
    CK(hipMalloc(&dCnt, LP_MAXB * 4)); CK(hipMalloc(&dStart, (LP_MAXB + 1) * 4)); CK(hipMalloc(&dCur, LP_MAXB * 4));
    CK(hipMalloc(&dFBeg, (size_t) nb1 * nb2 * 4)); CK(hipMalloc(&dFCnt, (size_t) nb1 * nb2 * 4)); CK(hipMalloc(&dRes, 24));
    CK(hipMalloc(&dPB, nP * 8)); CK(hipMalloc(&dPE, nP * 8)); CK(hipMalloc(&dRB, nb1 * 8)); CK(hipMalloc(&dRE, nb1 * 8));
    CK(hipMemcpy(dPB, pb.data(), nP * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dPE, pe.data(), nP * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dRB, rb.data(), nb1 * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dRE, re.data(), nb1 * 8, hipMemcpyHostToDevice));
    Timer tm; int fails = 0;
    auto tagged = [&](const uint32_t *tags, uint64_t n) { unsigned long long c = 0; CK(hipMemset(dRes + 2, 0, 8)); countTaggedKernel<<<numCU * 8, 256>>>(tags, n, dRes + 2); CK(hipMemcpy(&c, dRes + 2, 8, hipMemcpyDeviceToHost)); return c; };
    auto check = [&](const uint32_t *tags, uint64_t n, const uint32_t *beg, const uint32_t *cnt, const uint32_t *start, uint32_t nBuckets, unsigned long long expect) {
        unsigned long long r[2];
        CK(hipMemset(dSeen, 0, (n / 32 + 1) * 4)); CK(hipMemset(dRes, 0, 16));
        checkListKernel<<<numCU * 8, 256>>>(tags, n, dList, beg, cnt, start, nBuckets, dSeen, dRes);
        CK(hipMemcpy(r, dRes, 16, hipMemcpyDeviceToHost));
        const bool ok = r[0] == expect && r[1] == 0;
        printf("      check: %llu of %llu tagged lines listed once in their bucket's range, %llu bad entries: %s\n", r[0], expect, r[1], ok ? "verified" : "MISMATCH"); fflush(stdout);
        if (!ok) fails++;
    };
    for (int ks = 0; ks < 4; ks++) {
        if (only != "all" && only != KS_NAME[ks]) continue;
        printf("== key set %s\n", KS_NAME[ks]);
        genTagsKernel<<<numCU * 4, 256>>>(dTag1, dPB, dPE, nP, nb1 / 2, ks, nb1, 0);
        genTagsKernel<<<numCU * 4, 256>>>(dTag2, dRB, dRE, nb1, nb2 / 2, ks, nb2, 1);
        CK(hipDeviceSynchronize());
        const unsigned long long n1 = tagged(dTag1, cap1), n2 = tagged(dTag2, cap2);
        // ---- level 1 ----
        const double bytes1 = 4.0 * cap1 + 4.0 * n1;
        printf("-- level 1: %llu tags read, %llu list entries written\n", (unsigned long long) cap1, n1);
        tm.copyMs = 0;
        double c = tm.run("copy, dword per lane, 1024 threads x 2 per CU", bytes1, reps, [&] { copyTagsKernel<false><<<numCU * 2, 1024>>>(dTag1, dList, cap1); });
        c = std::min(c, tm.run("copy, dwordx4 per lane, 1024 threads x 2 per CU", bytes1, reps, [&] { copyTagsKernel<true><<<numCU * 2, 1024>>>(dTag1, dList, cap1); }));
        tm.copyMs = c;
        auto histScan = [&] {
            CK(hipMemsetAsync(dCnt, 0, LP_MAXB * 4, 0));
            hipLaunchKernelGGL(tagHistKernel, dim3(numCU * 8), dim3(256), 0, 0, (const uint32_t *) dTag1, cap1, nb1, dCnt);
            hipLaunchKernelGGL(tagScanKernel, dim3(1), dim3(1024), 0, 0, (const uint32_t *) dCnt, nb1, dStart, dCur);
        };
        tm.run("tagHistKernel + tagScanKernel (parent and change)", 4.0 * cap1, reps, histScan);
        tm.run("tagScatterKernel (parent)", bytes1, reps, [&] {
            CK(hipMemcpyAsync(dCur, dStart, LP_MAXB * 4, hipMemcpyDeviceToDevice, 0));
            hipLaunchKernelGGL(tagScatterKernel, dim3(numCU * 2), dim3(TS_BLOCK), 0, 0, (const uint32_t *) dTag1, cap1, nb1, dCur, dList); });
        check(dTag1, cap1, nullptr, nullptr, dStart, nb1, n1);
        if (!currentOnly) for (const ScatterV &v : SCATTER) {
            const size_t lds = listRunsLdsBytes(v.chunk, false);
            CK(hipFuncSetAttribute(reinterpret_cast<const void *>(v.k), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
            for (unsigned w = 1; w <= perCU(lds, v.block); w++) {
                char what[128]; snprintf(what, sizeof(what), "%s, %u per CU", v.name, w);
                CK(hipMemset(dList, 0xFF, cap1 * 4));
                tm.run(what, bytes1, reps, [&] {
                    CK(hipMemcpyAsync(dCur, dStart, LP_MAXB * 4, hipMemcpyDeviceToDevice, 0));
                    hipLaunchKernelGGL(v.k, dim3(numCU * w), dim3(v.block), lds, 0, (const uint32_t *) dTag1, cap1, nb1, dCur, dList); });
                check(dTag1, cap1, nullptr, nullptr, dStart, nb1, n1);
            }
        }
        // ---- level 2 ----
        const double bytes2 = 4.0 * cap2 + 4.0 * n2;
        printf("-- level 2: %llu tags read (the parent's kernel reads them twice), %llu list entries written\n", (unsigned long long) cap2, n2);
        tm.copyMs = 0;
        c = tm.run("copy, dword per lane, 1024 threads x 2 per CU", bytes2, reps, [&] { copyTagsKernel<false><<<numCU * 2, 1024>>>(dTag2, dList, cap2); });
        c = std::min(c, tm.run("copy, dwordx4 per lane, 1024 threads x 2 per CU", bytes2, reps, [&] { copyTagsKernel<true><<<numCU * 2, 1024>>>(dTag2, dList, cap2); }));
        tm.copyMs = c;
        CK(hipMemset(dList, 0xFF, cap2 * 4));
        tm.run("tagSortRegionKernel (parent)", bytes2, reps, [&] {
            hipLaunchKernelGGL(tagSortRegionKernel, dim3(std::min<uint32_t>(nb1, numCU * 4)), dim3(512), 0, 0, (const uint32_t *) dTag2, (const uint64_t *) dRB, (const uint64_t *) dRE, nb1, nb2, dList, dFBeg, dFCnt); });
        check(dTag2, cap2, dFBeg, dFCnt, nullptr, nb1 * nb2, n2);
        if (!currentOnly) for (const RegionV &v : REGION) {
            const size_t lds = listRunsLdsBytes(v.chunk, true);
            CK(hipFuncSetAttribute(reinterpret_cast<const void *>(v.k), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
            for (unsigned w = 1; w <= perCU(lds, v.block); w++) {
                char what[128]; snprintf(what, sizeof(what), "%s, %u per CU", v.name, w);
                CK(hipMemset(dList, 0xFF, cap2 * 4)); CK(hipMemset(dFBeg, 0xFF, (size_t) nb1 * nb2 * 4)); CK(hipMemset(dFCnt, 0, (size_t) nb1 * nb2 * 4));
                tm.run(what, bytes2, reps, [&] {
                    hipLaunchKernelGGL(v.k, dim3(std::min<uint32_t>(nb1, numCU * w)), dim3(v.block), lds, 0, (const uint32_t *) dTag2, (const uint64_t *) dRB, (const uint64_t *) dRE, nb1, nb2, dList, dFBeg, dFCnt); });
                check(dTag2, cap2, dFBeg, dFCnt, nullptr, nb1 * nb2, n2);
            }
        }
    }
    printf("linelist_bench: %d failing checks\n", fails);
    return fails ? 1 : 0;
}
