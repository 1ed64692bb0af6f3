// Device utilities shared by the plasship kernels: wave64 reductions/scans and a device-wide
// exclusive scan.  gfx950 only: wavefront = 64 lanes, hard-coded.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace plasship {

constexpr int WAVE = 64;

__device__ __forceinline__ int laneId() { return (int) (threadIdx.x & 63); }

// ---- DPP row operations (a row = 16 consecutive lanes): cross-lane moves on the VALU, no LDS crossbar ----
// ctrl: quad_perm 0x00-0xFF, row_ror:n 0x120+n, row_mirror 0x140, row_half_mirror 0x141
template <int CTRL> __device__ __forceinline__ uint32_t dppMov(uint32_t v) {
    return (uint32_t) __builtin_amdgcn_mov_dpp((int) v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ unsigned long long dppMov64(unsigned long long v) {
    const uint32_t lo = dppMov<CTRL>((uint32_t) v), hi = dppMov<CTRL>((uint32_t) (v >> 32));
    return ((unsigned long long) hi << 32) | lo;
}
// all-reduce over each row of W = 16 lanes, or over each half row of W = 8: xor 1, xor 2 (quad_perm), mirror inside 8, then mirror inside 16
// (the first three steps stay inside the aligned eight lanes, so the half-row forms are the row forms without their last step)
template <int W> __device__ __forceinline__ int rowSum(int v) {
    static_assert(W == 8 || W == 16, "a row of 16 lanes or half of one");
    v += (int) dppMov<0xB1>((uint32_t) v); v += (int) dppMov<0x4E>((uint32_t) v);
    v += (int) dppMov<0x141>((uint32_t) v);
    if (W == 16) v += (int) dppMov<0x140>((uint32_t) v);
    return v;
}
template <int W> __device__ __forceinline__ unsigned long long rowMax(unsigned long long v) {
    static_assert(W == 8 || W == 16, "a row of 16 lanes or half of one");
    unsigned long long o;
    o = dppMov64<0xB1>(v); v = o > v ? o : v;
    o = dppMov64<0x4E>(v); v = o > v ? o : v;
    o = dppMov64<0x141>(v); v = o > v ? o : v;
    if (W == 16) { o = dppMov64<0x140>(v); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int rowSum16(int v) { return rowSum<16>(v); }
__device__ __forceinline__ unsigned long long rowMax16(unsigned long long v) { return rowMax<16>(v); }
__device__ __forceinline__ uint32_t rowMin16U32(uint32_t v) {
    uint32_t o;
    o = dppMov<0xB1>(v); v = o < v ? o : v;
    o = dppMov<0x4E>(v); v = o < v ? o : v;
    o = dppMov<0x141>(v); v = o < v ? o : v;
    o = dppMov<0x140>(v); v = o < v ? o : v;
    return v;
}
__device__ __forceinline__ uint32_t rowOr16(uint32_t v) {
    v |= dppMov<0xB1>(v); v |= dppMov<0x4E>(v); v |= dppMov<0x141>(v); v |= dppMov<0x140>(v);
    return v;
}
// number of lanes in the own row of 16 whose value is smaller than `mine` (own lane excluded by the strict compare
// when other == mine); `other` is the value to rotate: the own value, or another row's value fetched by a shuffle
template <int N> struct RowCountLess {
    static __device__ __forceinline__ uint32_t run(uint32_t other, uint32_t mine) {
        return ((dppMov<0x120 + N>(other) < mine) ? 1u : 0u) + RowCountLess<N - 1>::run(other, mine);
    }
};
template <> struct RowCountLess<0> { static __device__ __forceinline__ uint32_t run(uint32_t, uint32_t) { return 0u; } };
__device__ __forceinline__ uint32_t rowCountLess16(uint32_t other, uint32_t mine, bool includeUnrotated) {
    return RowCountLess<15>::run(other, mine) + ((includeUnrotated && other < mine) ? 1u : 0u);
}

// the same over a half row of 8 lanes (row_ror would cross into the other half): the three rotations of the own quad, then the other
// quad by way of the half row's mirror image and its three rotations — seven compares
__device__ __forceinline__ uint32_t rowCountLess8(uint32_t mine) {
    const uint32_t far = dppMov<0x141>(mine);
    return ((dppMov<0x39>(mine) < mine) ? 1u : 0u) + ((dppMov<0x4E>(mine) < mine) ? 1u : 0u) + ((dppMov<0x93>(mine) < mine) ? 1u : 0u) +
           ((far < mine) ? 1u : 0u) + ((dppMov<0x39>(far) < mine) ? 1u : 0u) + ((dppMov<0x4E>(far) < mine) ? 1u : 0u) + ((dppMov<0x93>(far) < mine) ? 1u : 0u);
}

__device__ __forceinline__ int waveReduceSum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long waveReduceSumU64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int waveReduceMax(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// inclusive prefix sum across the wave
__device__ __forceinline__ unsigned waveInclusiveScan(unsigned v) {
    const int l = laneId();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { unsigned t = __shfl_up(v, o, 64); if (l >= o) v += t; }
    return v;
}
__device__ __forceinline__ unsigned long long waveInclusiveScanU64(unsigned long long v) {
    const int l = laneId();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { unsigned long long t = __shfl_up(v, o, 64); if (l >= o) v += t; }
    return v;
}

// ---- 8 bytes at any address (gfx950 global loads / stores take unaligned addresses) ----
__device__ __forceinline__ uint64_t loadU64Unaligned(const char *p) { uint64_t w; __builtin_memcpy(&w, p, 8); return w; }
__device__ __forceinline__ void storeU64Unaligned(char *p, uint64_t w) { __builtin_memcpy(p, &w, 8); }
// the last, partial word of a copy: the low r = 1-7 bytes of v as one 4-, 2- and 1-byte store each, never a byte beyond d + r
// (byte by byte the tail was up to seven stores of the whole wavefront per copy: round 3, profiles/r03_pmc)
__device__ __forceinline__ void storeTail(char *d, uint64_t v, unsigned r) {
    if (r & 4u) { const uint32_t x = (uint32_t) v; __builtin_memcpy(d, &x, 4); d += 4; v >>= 32; }
    if (r & 2u) { const uint16_t x = (uint16_t) v; __builtin_memcpy(d, &x, 2); d += 2; v >>= 16; }
    if (r & 1u) *d = (char) v;
}

// ---- device-wide exclusive scan of uint32 counts into uint64 offsets ------------------------------
// out[i] = sum_{j<i} in[j], out[n] = total.  Three-kernel scheme (reduce / scan partials / downsweep);
// the partial array is scanned recursively.  Traffic 12 B/element read + 8 B written: negligible next
// to the record arrays it indexes.
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 8;                       // per thread
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;  // 2048 elements per block

int exclusiveScanU32(hipStream_t stream, const uint32_t *d_in, uint64_t *d_out, size_t n, void *d_tmp, size_t tmpBytes);
size_t exclusiveScanTmpBytes(size_t n);
// same, input already uint64 (in place allowed: d_in == d_out)
int exclusiveScanU64(hipStream_t stream, const uint64_t *d_in, uint64_t *d_out, size_t n, void *d_tmp, size_t tmpBytes);

}  // namespace plasship
