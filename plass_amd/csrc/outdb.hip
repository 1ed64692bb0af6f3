// plasship: the output-DB writer.  Product code.  Every module that derives a sequence DB from another one goes through buildOutputDB
// (assembleresults and its nucleotide and guided variants, cyclecheck, findassemblystart); packedCopyOf lays a DB that lives in a
// shared heap out like its data file.  The shared heap (SeqHeap), the lineage (parentGen / ancestorGen / d_changed) and the origin
// (originGen / d_origin) that kmermatcher's two caches and cyclecheck's known-linear entries rest on are recorded here and nowhere else.
#include "common.hpp"
#include "device_utils.hpp"
#include <algorithm>
#include <memory>

namespace plasship {

__global__ void outLenKernel(SeqView s, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ newLen, int keepTarget,
                             uint64_t *__restrict__ outBytes, uint32_t *__restrict__ keep, uint64_t *__restrict__ appBytes) {
    for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < s.n; id += gridDim.x * blockDim.x) {
        const uint32_t f = flags[id];
        uint64_t b = 0, ap = 0; uint32_t k = 0;
        if (f & 0x20u) { b = (uint64_t) newLen[id] + 2; k = 1; ap = b; }
        else if (keepTarget || !(f & 0x80u)) { b = (uint64_t) s.len[id] + 2; k = 1; }
        outBytes[id] = b; keep[id] = k;
        if (appBytes) appBytes[id] = ap;                      // what the entry adds to a shared heap: only rewritten entries have new bytes
    }
}

// The output DB as an INDEX over the heap the input DB lives in (SeqHeap, common.hpp): an entry that is carried over keeps its bytes
// where they are, a rewritten one (flag 0x20: extended, cut, chopped) is copied from the arena to heapBase + appOff[id] behind
// everything the heap held.  G lanes per entry; what moves per iteration is the rewritten 10-20 % of the sequences instead of
// 2 x all residues (writeOutKernel below: 15 ms per iteration at 50 M reads, the same again on every rank of a sharded run).
// Round 5: ONE THREAD per entry for the index (coalesced: rounds 4's eight lanes per entry read every index word eight times over and moved
// 14.6 + 5.4 GB per launch for ~3 GB of rewritten entries), then the wavefront copies the rewritten entries of its 64 ids one after the other
// with all 64 lanes, 8 bytes per lane and step (a rewritten entry is a contig of a few hundred residues: one to three steps).
__global__ __launch_bounds__(256) void appendOutKernel(SeqView s, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ newLen,
                                                       const uint64_t *__restrict__ newStart, const char *arena,
                                                       const uint64_t *__restrict__ appOff, uint64_t heapBase, const uint32_t *__restrict__ keep,
                                                       const uint64_t *__restrict__ keepPos, const uint32_t *__restrict__ inKey,
                                                       char *heap, uint64_t *__restrict__ outOffArr, uint32_t *__restrict__ outLen, uint32_t *__restrict__ outKey,
                                                       unsigned char *__restrict__ changedOut) {
    // (arena and heap are NOT restrict: cyclecheck and findassemblystart pass the heap itself as the arena — disjoint ranges of one buffer)
    const int lane = laneId();
    for (uint32_t id0 = (blockIdx.x * 256 + (threadIdx.x & ~63u)); id0 < s.n; id0 += gridDim.x * 256) {
        const uint32_t id = id0 + (uint32_t) lane;
        bool ext = false; uint32_t L = 0; uint64_t srcOff = 0, o = 0;
        if (id < s.n && keep[id]) {
            ext = (flags[id] & 0x20u) != 0;
            if (ext) { L = newLen[id]; o = heapBase + appOff[id]; srcOff = newStart[id]; }
            else { L = s.len[id]; o = s.off[id]; }
            const uint64_t j = keepPos[id];
            outOffArr[j] = o; outLen[j] = L; outKey[j] = inKey[id];
            if (changedOut) changedOut[j] = ext ? 1 : 0;
        }
        unsigned long long m = __ballot(ext);
        while (m) {
            const int src = __ffsll((long long) m) - 1;
            m &= m - 1;
            const uint32_t cl = (uint32_t) __shfl((int) L, src, 64);
            const uint64_t co = (uint64_t) __shfl((unsigned long long) o, src, 64), cs = (uint64_t) __shfl((unsigned long long) srcOff, src, 64);
            const char *from = arena + cs; char *dst = heap + co;
            for (unsigned p = 8u * (unsigned) lane; p < cl; p += 512u) {
                const uint64_t x = loadU64Unaligned(from + p);                           // buffers are padded past their ends
                if (p + 8 <= cl) storeU64Unaligned(dst + p, x); else storeTail(dst + p, x, cl - p);
            }
            if (lane == 0) { dst[cl] = '\n'; dst[cl + 1] = '\0'; }
        }
    }
}

// origin of every entry of an output DB in the anchor DB of kmermatcher's position cache (plasship_seqdb::d_origin; round 6): a carried-over
// entry keeps the id its source had there (the source's own id when the source IS the anchor), a rewritten entry has none
__global__ __launch_bounds__(256) void originOutKernel(uint32_t n, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ keepPos,
                                                       const uint32_t *__restrict__ srcOrigin, uint32_t *__restrict__ outOrigin) {
    for (uint32_t id = blockIdx.x * 256 + threadIdx.x; id < n; id += gridDim.x * 256)
        if (keep[id]) outOrigin[keepPos[id]] = (flags[id] & 0x20u) ? 0xFFFFFFFFu : (srcOrigin ? srcOrigin[id] : id);
}

template <int G, int U>
__global__ __launch_bounds__(256) void writeOutKernel(SeqView s, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ newLen,
                                                      const uint64_t *__restrict__ newStart, const char *__restrict__ arena,
                                                      const uint64_t *__restrict__ outOff, const uint32_t *__restrict__ keep,
                                                      const uint64_t *__restrict__ keepPos, const uint32_t *__restrict__ inKey,
                                                      char *__restrict__ outData, uint64_t *__restrict__ outOffArr, uint32_t *__restrict__ outLen, uint32_t *__restrict__ outKey,
                                                      unsigned char *__restrict__ changedOut) {
    // G lanes per sequence, 8 bytes per lane and step: 8 lanes take a read fragment (~46 residues) in one step with most lanes busy,
    // eight sequences per wavefront; contigs take a few steps of contiguous 64-byte pieces.  A sequence is a chain of dependent
    // round trips (what to copy -> the bytes -> the store) and the kernel is bound by the number of chains in flight (round 3: the
    // wavefronts were parked on memory 89 % of their cycles at 2 TB/s), so a group works on U sequences at a time: the U sets of
    // metadata are requested together, then the U first pieces.
    const int gl = threadIdx.x & (G - 1);
    constexpr int groupsPerBlock = 256 / G;
    const uint32_t stride = gridDim.x * groupsPerBlock;
    for (uint32_t id0 = blockIdx.x * groupsPerBlock + (threadIdx.x / G); id0 < s.n; id0 += stride * U) {
        uint32_t L[U]; const char *src[U]; uint64_t o[U]; bool k[U]; uint64_t w[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t id = id0 + (uint32_t) u * stride;
            k[u] = id < s.n && keep[id] != 0;
            L[u] = 0; src[u] = s.data; o[u] = 0;
            if (k[u]) {
                const uint32_t f = flags[id]; const uint32_t l0 = s.len[id]; const uint64_t o0 = s.off[id];
                o[u] = outOff[id];
                const bool ext = (f & 0x20u) != 0;
                L[u] = ext ? newLen[id] : l0;
                src[u] = ext ? (arena + newStart[id]) : (s.data + o0);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) w[u] = (k[u] && 8u * (unsigned) gl < L[u]) ? loadU64Unaligned(src[u] + 8 * gl) : 0ULL;     // buffers are padded past their ends
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!k[u]) continue;
            const uint32_t id = id0 + (uint32_t) u * stride;
            const unsigned i = 8u * (unsigned) gl;
            char *dst = outData + o[u];
            if (i + 8 <= L[u]) storeU64Unaligned(dst + i, w[u]);
            else if (i < L[u]) storeTail(dst + i, w[u], L[u] - i);
            for (unsigned p = i + 8u * G; p < L[u]; p += 8u * G) {                       // the rest of a contig
                const uint64_t x = loadU64Unaligned(src[u] + p);
                if (p + 8 <= L[u]) storeU64Unaligned(dst + p, x);
                else storeTail(dst + p, x, L[u] - p);
            }
            if (gl == 0) {
                dst[L[u]] = '\n'; dst[L[u] + 1] = '\0';
                const uint64_t j = keepPos[id];
                outOffArr[j] = o[u]; outLen[j] = L[u]; outKey[j] = inKey[id];
                if (changedOut) changedOut[j] = (flags[id] & 0x20u) ? 1 : 0;
            }
        }
    }
}

__global__ void maxU32Kernel(const uint32_t *__restrict__ v, uint64_t n, uint32_t *__restrict__ out) {
    uint32_t m = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) m = max(m, v[i]);
    m = (uint32_t) waveReduceMax((int) m);
    if (laneId() == 0) atomicMax(out, m);
}

// what an OutPlacement (common.hpp) decides, stated once
struct PlacementRules {
    bool lineage;         // d_changed, parentGen / ancestorGen and the origin are recorded
    bool heaps;           // the DB shares its parent's heap when that has one with room, else opens a heap of its own; false (Exact and Packed, always): an exact buffer
};
static PlacementRules rulesOf(OutPlacement p) {
    return {p != OutPlacement::Packed, p == OutPlacement::Chain && tuneInt("DBHEAP", 1) == 1};
}

}  // namespace plasship
using namespace plasship;

// Shares `db`'s heap when the placement allows it and the heap has room (appendOutKernel: only the rewritten entries move); else the
// entries are written back to back (writeOutKernel) into a NEW heap with room for the iterations to come (as much again as the data,
// at most PLASSHIP_TUNE_DBHEAP_GB = 16 GB) or, where the placement has no heaps, into an exact buffer of the DB's own.
int plasship::buildOutputDB(plasship_ctx *ctx, const plasship_seqdb *db, const OutEdits &ed, void *dTmp, size_t tmpBytes, plasship_seqdb **out, const OutOptions &opt) {
    hipStream_t st = ctx->stream;
    const uint32_t N = (uint32_t) db->n;
    const SeqView sv = db->view();
    const PlacementRules rules = rulesOf(opt.placement);
    const bool mayAppend = rules.heaps && db->heap != nullptr;
    DevBuf dOutBytes, dKeep, dOutOff, dKeepPos, dMaxLen, dAppBytes, dAppOff;
    if (dOutBytes.alloc(((size_t) N + 1) * 8) != hipSuccess || dKeep.alloc(((size_t) N + 1) * 4) != hipSuccess || dOutOff.alloc(((size_t) N + 2) * 8) != hipSuccess ||
        dKeepPos.alloc(((size_t) N + 2) * 8) != hipSuccess || dMaxLen.alloc(4) != hipSuccess ||
        (mayAppend && (dAppBytes.alloc(((size_t) N + 1) * 8) != hipSuccess || dAppOff.alloc(((size_t) N + 2) * 8) != hipSuccess))) { setError("plasship_assemble: out of device memory"); return PLASSHIP_ERR_DEVICE; }
    if (N) hipLaunchKernelGGL(outLenKernel, dim3(std::min<uint32_t>((N + 255) / 256, 8192)), dim3(256), 0, st, sv, ed.flags, ed.newLen, ed.keepTarget, dOutBytes.as<uint64_t>(), dKeep.as<uint32_t>(),
                              mayAppend ? dAppBytes.as<uint64_t>() : (uint64_t *) nullptr);
    if (exclusiveScanU64(st, dOutBytes.as<uint64_t>(), dOutOff.as<uint64_t>(), N, dTmp, tmpBytes) ||
        exclusiveScanU32(st, dKeep.as<uint32_t>(), dKeepPos.as<uint64_t>(), N, dTmp, tmpBytes) ||
        (mayAppend && exclusiveScanU64(st, dAppBytes.as<uint64_t>(), dAppOff.as<uint64_t>(), N, dTmp, tmpBytes))) { setError("plasship_assemble: scan failed"); return PLASSHIP_ERR_DEVICE; }
    uint64_t outBytes = 0, outN = 0, appTotal = 0;
    PH_CHECK(hipMemcpyAsync(&outBytes, dOutOff.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    PH_CHECK(hipMemcpyAsync(&outN, dKeepPos.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    if (mayAppend) PH_CHECK(hipMemcpyAsync(&appTotal, dAppOff.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    PH_CHECK(plasship::streamSync(st));
    PH_CHECK(hipGetLastError());
    std::unique_ptr<plasship_seqdb> holder(new plasship_seqdb());   // released to the caller on success only
    plasship_seqdb *o = holder.get();
    o->dbtype = db->dbtype; o->n = (size_t) outN; o->dataBytes = outBytes; o->residues = outBytes - 2 * outN; o->hostIndexValid = false;
    if (o->d_off.allocLong((outN + 1) * 8) != hipSuccess || o->d_len.allocLong((outN + 1) * 4) != hipSuccess || o->d_key.allocLong((outN + 1) * 4) != hipSuccess) {
        setError("plasship_assemble: out of device memory for the output DB's index"); return PLASSHIP_ERR_DEVICE;
    }
    // lineage: the extended / cut entries marked (one byte per NEW id); same ids as `db` if nothing was dropped (kmermatcher's
    // selected-window cache needs that), else only "an unmarked entry is an entry of `db`" (cyclecheck's known-linear entries)
    if (outN && rules.lineage) {
        if (o->d_changed.allocLong((size_t) outN) != hipSuccess) { setError("plasship_assemble: out of device memory"); return PLASSHIP_ERR_DEVICE; }
        o->ancestorGen = db->gen;
        if (outN == N) o->parentGen = db->gen;
    }
    // ... and, when `db` is the anchor of kmermatcher's position cache or descends from it, the id every carried-over entry had in the anchor
    if (outN && rules.lineage && ctx->kmPosCache.valid && ctx->kmPosCache.gen != 0) {
        const uint64_t anchor = ctx->kmPosCache.gen;
        const bool isAnchor = db->gen == anchor, descends = !isAnchor && db->originGen == anchor && db->d_origin.p != nullptr;
        if (isAnchor || descends) {
            if (o->d_origin.allocLong((size_t) outN * 4) != hipSuccess) { setError("plasship_assemble: out of device memory"); return PLASSHIP_ERR_DEVICE; }
            o->originGen = anchor;
            hipLaunchKernelGGL(originOutKernel, dim3(std::min<uint32_t>((N + 255) / 256, 4096)), dim3(256), 0, st, N, ed.flags, (const uint32_t *) dKeep.as<uint32_t>(), (const uint64_t *) dKeepPos.as<uint64_t>(),
                               descends ? (const uint32_t *) db->d_origin.as<uint32_t>() : (const uint32_t *) nullptr, o->d_origin.as<uint32_t>());
        }
    }
    // room in the shared heap?  (the reservation is atomic: two DBs derived from one parent get disjoint ranges)
    bool append = false; uint64_t heapBase = 0;
    if (mayAppend) {                                          // (the reservation commits only if it fits: a DB that does not fit leaves the heap's room to its siblings)
        uint64_t cur = db->heap->used.load();
        while (cur + appTotal + 64 <= db->heap->buf.bytes) {
            if (db->heap->used.compare_exchange_weak(cur, cur + appTotal)) { heapBase = cur; append = true; break; }
        }
    }
    if (append) {
        o->heap = db->heap; o->contiguous = false;
        if (N) hipLaunchKernelGGL(appendOutKernel, dim3(std::min<uint32_t>((N + 255) / 256, (uint32_t) ctx->numCU * 16u)), dim3(256), 0, st, sv, ed.flags, ed.newLen, ed.newStart, ed.arena,
                                  (const uint64_t *) dAppOff.as<uint64_t>(), heapBase, (const uint32_t *) dKeep.as<uint32_t>(), (const uint64_t *) dKeepPos.as<uint64_t>(), (const uint32_t *) db->d_key.as<uint32_t>(),
                                  db->heap->buf.as<char>(), o->d_off.as<uint64_t>(), o->d_len.as<uint32_t>(), o->d_key.as<uint32_t>(), o->d_changed.as<unsigned char>());
    } else {
        char *dst = nullptr;
        if (rules.heaps) {
            o->heap = std::make_shared<SeqHeap>();
            // room for the entries the next iterations rewrite (25-35 % of the data per iteration at 50 M reads): as much again as the
            // data, but no more than PLASSHIP_TUNE_DBHEAP_GB (default 16; round 4: 8 — the sparse alignment lists of round 5 freed 14 GB) — kmermatcher's record arrays need 170 of the 288 GB there
            const uint64_t cap = outBytes + std::min<uint64_t>(outBytes, (uint64_t) tuneInt("DBHEAP_GB", 16) << 30) + 4096;
            if (o->heap->buf.allocLong(cap) == hipSuccess) { o->heap->used = outBytes; dst = o->heap->buf.as<char>(); }
            else o->heap.reset();                             // no room for the slack: an exact buffer will do
        }
        if (!dst) {
            if (o->d_data.allocLong(outBytes + 64) != hipSuccess) {
                size_t fr = 0, tt = 0; (void) hipMemGetInfo(&fr, &tt);
                setError("plasship_assemble: out of device memory for the output DB (" + std::to_string(outBytes) + " bytes, " + std::to_string(outN) + " sequences; device free " + std::to_string(fr) + " of " + std::to_string(tt) + ")"); return PLASSHIP_ERR_DEVICE;
            }
            dst = o->d_data.as<char>();
        }
        o->contiguous = true;
        PH_CHECK(hipMemsetAsync(dst + outBytes, 0, 64, st));
        if (N) {
            // (2 and 4 sequences in flight per lane group changed nothing — profiles/r03_ab_knobs.txt: the kernel is not bound by its chains of round trips.
            //  U stays a template parameter: written out as straight code the kernel compiles to other instructions)
            const unsigned woGrid = std::min<uint32_t>((N + 15) / 16, (uint32_t) ctx->numCU * 16u);
            hipLaunchKernelGGL((writeOutKernel<8, 1>), dim3(woGrid), dim3(256), 0, st, sv, ed.flags, ed.newLen,
                               ed.newStart, ed.arena, dOutOff.as<uint64_t>(), dKeep.as<uint32_t>(), dKeepPos.as<uint64_t>(), db->d_key.as<uint32_t>(),
                               dst, o->d_off.as<uint64_t>(), o->d_len.as<uint32_t>(), o->d_key.as<uint32_t>(), o->d_changed.as<unsigned char>());
        }
    }
    PH_CHECK(hipMemcpyAsync(o->d_off.as<uint64_t>() + outN, &outBytes, 8, hipMemcpyHostToDevice, st));
    PH_CHECK(hipMemsetAsync(dMaxLen.p, 0, 4, st));
    if (outN) hipLaunchKernelGGL(maxU32Kernel, dim3(std::min<uint64_t>((outN + 255) / 256, 1024)), dim3(256), 0, st, o->d_len.as<uint32_t>(), outN, dMaxLen.as<uint32_t>());
    uint32_t maxLen = 0;
    if (opt.doneEvent) PH_CHECK(hipEventRecord(opt.doneEvent, st));
    PH_CHECK(hipMemcpyAsync(&maxLen, dMaxLen.p, 4, hipMemcpyDeviceToHost, st));
    if (opt.dExtra) PH_CHECK(hipMemcpyAsync(opt.hExtra, opt.dExtra, opt.extraBytes, hipMemcpyDeviceToHost, st));      // the caller's counters ride along
    PH_CHECK(plasship::streamSync(st));
    PH_CHECK(hipGetLastError());
    o->maxEntryLen = maxLen + 2;
    o->buildAppendedBytes = append ? appTotal : 0; o->buildCopiedBytes = append ? 0 : outBytes;
    *out = holder.release();
    return PLASSHIP_OK;
}

int plasship::packedCopyOf(plasship_ctx *ctx, const plasship_seqdb *db, std::unique_ptr<plasship_seqdb> &out) {
    const uint32_t N = (uint32_t) db->n;
    DevBuf dFlags, dTmp; const size_t tmpBytes = exclusiveScanTmpBytes((size_t) N + 2);
    if (dFlags.alloc(((size_t) N + 1) * 4) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess) { setError("plasship: out of device memory while packing a sequence DB"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync(dFlags.p, 0, ((size_t) N + 1) * 4, ctx->stream));
    plasship_seqdb *o = nullptr;
    const int rc = buildOutputDB(ctx, db, {.flags = dFlags.as<uint32_t>(), .keepTarget = 1}, dTmp.p, tmpBytes, &o, {.placement = OutPlacement::Packed});
    if (rc) return rc;
    o->maxEntryLen = db->maxEntryLen;
    out.reset(o);
    return PLASSHIP_OK;
}
