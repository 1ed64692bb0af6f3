// plasship: result2repseq on gfx950 — the representatives' sequences of a clustering as a sequence DB.  Product code, built into the extension
// library libplasship_subst.so (include/plasship_ext/subst.h).  What a user wants from redundancy reduction: the step that follows linclust in
// data/guidedNuclAssemble.sh:182-186.
//
// Reference behaviour reproduced (lib/mmseqs/src/util/result2repseq.cpp:37-49): for every entry of the cluster DB the sequence of the FIRST key
// on its list, stored under the entry's key; an empty entry gives no output entry; the output has the sequence DB's type.  Clustering::writeData
// and mergeclusters put a cluster's own key first (pairListWrite in clust.hip, the places of merge_clusters.hip), so the first key is the entry's key: the output is the
// subset of the representatives, which a clustering names by repOf[id] == id and a merged clustering by the representatives of its pairs.
// Three flat kernels and two scans: mark, place (index and byte offset are exclusive scans of the marks and of the marked entry lengths),
// copy (one wavefront per entry, 16 bytes per lane and step from wherever the source entry lies; the tail byte by byte — no load leaves
// the entry).  Every id is bounds-checked against the DB before it is used.
// Algorithmic bytes: 8 or 4 per sequence (pair or repOf) + 12 (offset, length) read, 2 * entry bytes per representative moved.
#include "common.hpp"
#include "../../include/plasship_ext/subst.h"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <cstring>
#include <memory>

namespace plasship {

__global__ void repMarkClustersKernel(const uint32_t *__restrict__ repOf, uint32_t n, uint32_t *__restrict__ mark) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) mark[i] = repOf[i] == (uint32_t) i ? 1u : 0u;
}
// (mark is zeroed before; a representative is named by every pair of its cluster: the same value is stored)
__global__ void repMarkMergedKernel(const uint64_t *__restrict__ pairs, uint32_t n, uint32_t *__restrict__ mark, unsigned long long *bad) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t rep = (uint32_t) (pairs[j] >> 32);
        if (rep >= n) { atomicAdd(bad, 1ull); continue; }
        if (j == 0 || (uint32_t) (pairs[j - 1] >> 32) != rep) mark[rep] = 1u;
    }
}
__global__ void repBytesKernel(const uint32_t *__restrict__ mark, const uint32_t *__restrict__ len, uint32_t n, uint32_t *__restrict__ bytes) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) bytes[i] = mark[i] ? len[i] + 2u : 0u;
}
// one wavefront per marked entry: the index lines of the output and the entry's bytes ("SEQ\n\0": len + 2)
__global__ __launch_bounds__(256) void repGatherKernel(SeqView db, const uint32_t *__restrict__ key, const uint32_t *__restrict__ mark, const uint64_t *__restrict__ place,
                                                       const uint64_t *__restrict__ pos, uint64_t nOut, uint64_t outBytes, char *__restrict__ outData, uint64_t *__restrict__ outOff,
                                                       uint32_t *__restrict__ outLen, uint32_t *__restrict__ outKey, unsigned long long *bad) {
    const unsigned lane = (unsigned) laneId();
    const uint64_t waves = (uint64_t) gridDim.x * (blockDim.x / WAVE);
    for (uint64_t i = (uint64_t) blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; i < db.n; i += waves) {
        if (!mark[i]) continue;
        const uint64_t e = place[i], o = pos[i];
        const uint32_t l = db.len[i], nb = l + 2u;
        if (e >= nOut || o + nb > outBytes) { if (lane == 0) atomicAdd(bad, 1ull); continue; }
        if (lane == 0) { outOff[e] = o; outLen[e] = l; outKey[e] = key[i]; }
        const char *src = db.data + db.off[i];
        char *dst = outData + o;
        const uint32_t nFull = nb & ~15u;
        for (uint32_t b = 16u * lane; b < nFull; b += 16u * WAVE) { uint32_t w[4]; __builtin_memcpy(w, src + b, 16); __builtin_memcpy(dst + b, w, 16); }
        if (lane < nb - nFull) dst[nFull + lane] = src[nFull + lane];
    }
}

// the marked entries of `db` as a DB of their own; dMark: uint32 [n]
static int gatherMarked(plasship_ctx *ctx, const char *what, const plasship_seqdb *db, const uint32_t *dMark, plasship_seqdb **out) {
    const uint32_t n = (uint32_t) db->n;
    const size_t tmpBytes = exclusiveScanTmpBytes(n);
    DevBuf dBytes, dPlace, dPos, dTmp, dBad;
    if (dBytes.alloc((size_t) n * 4) != hipSuccess || dPlace.alloc(((size_t) n + 1) * 8) != hipSuccess || dPos.alloc(((size_t) n + 1) * 8) != hipSuccess ||
        dTmp.alloc(tmpBytes) != hipSuccess || dBad.alloc(8) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync(dBad.p, 0, 8, ctx->stream));
    uint64_t ends[2] = {0, 0};
    if (n) {
        hipLaunchKernelGGL(repBytesKernel, dim3(flatGrid(n, ctx->numCU)), dim3(256), 0, ctx->stream, dMark, db->d_len.as<uint32_t>(), n, dBytes.as<uint32_t>());
        if (exclusiveScanU32(ctx->stream, dMark, dPlace.as<uint64_t>(), n, dTmp.p, tmpBytes) ||
            exclusiveScanU32(ctx->stream, dBytes.as<uint32_t>(), dPos.as<uint64_t>(), n, dTmp.p, tmpBytes)) { (void) plasship::streamSync(ctx->stream); setError(std::string(what) + ": scan failed"); return PLASSHIP_ERR_DEVICE; }
        PH_CHECK(hipMemcpyAsync(&ends[0], dPlace.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_CHECK(hipMemcpyAsync(&ends[1], dPos.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    PH_CHECK(plasship::streamSync(ctx->stream));
    const uint64_t nOut = ends[0], outBytes = ends[1];
    std::unique_ptr<plasship_seqdb> holder(new plasship_seqdb());     // released to the caller on success only
    plasship_seqdb *o = holder.get();
    o->dbtype = db->dbtype; o->n = (size_t) nOut; o->dataBytes = outBytes; o->residues = outBytes - 2 * nOut; o->hostIndexValid = false;
    // (padded like an uploaded DB, so that 16-byte loads at the tail of the last entry stay in bounds)
    if (o->d_data.allocLong(outBytes + 64) != hipSuccess || o->d_off.allocLong((nOut + 1) * 8) != hipSuccess || o->d_len.allocLong((nOut + 1) * 4) != hipSuccess ||
        o->d_key.allocLong((nOut + 1) * 4) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync(o->d_data.as<char>() + outBytes, 0, 64, ctx->stream));
    PH_CHECK(hipMemcpyAsync(o->d_off.as<uint64_t>() + nOut, &outBytes, 8, hipMemcpyHostToDevice, ctx->stream));
    const unsigned gw = (unsigned) std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t) n + 3) / 4, (uint64_t) ctx->numCU * 16));
    if (n) hipLaunchKernelGGL(repGatherKernel, dim3(gw), dim3(256), 0, ctx->stream, db->view(), db->d_key.as<uint32_t>(), dMark, dPlace.as<uint64_t>(), dPos.as<uint64_t>(), nOut, outBytes,
                       o->d_data.as<char>(), o->d_off.as<uint64_t>(), o->d_len.as<uint32_t>(), o->d_key.as<uint32_t>(), dBad.as<unsigned long long>());
    unsigned long long hb = 0;
    PH_CHECK(hipMemcpyAsync(&hb, dBad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hb) { setError(std::string(what) + ": internal error: an entry does not fit its place"); return PLASSHIP_ERR_DEVICE; }
    // the longest entry: the lengths of the output, once, on the host (4 bytes per representative; the caller writes or downloads the DB anyway)
    std::vector<uint32_t> lens(nOut);
    if (nOut) { const int rc = stagedCopyToHost(ctx, lens.data(), o->d_len.p, nOut * 4); if (rc) return rc; }
    uint32_t mx = 0; for (uint32_t l : lens) mx = std::max(mx, l);
    o->maxEntryLen = nOut ? mx + 2 : 0;
    *out = holder.release();
    return PLASSHIP_OK;
}

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_clusters_repseqs(plasship_ctx *ctx, const plasship_clusters *cl, const plasship_seqdb *db, plasship_seqdb **out) {
    const char *what = "plasship_clusters_repseqs";
    if (!ctx || !cl || !db || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (const int rc = refuseForeign(what, cl, db)) return rc;
    if (const int rc = refuseWideIds(what, db)) return rc;
    PH_ENTER(ctx);
    const uint32_t n = (uint32_t) db->n;
    DevBuf dMark;
    if (dMark.alloc(std::max<size_t>(n, 1) * 4) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
    if (n) hipLaunchKernelGGL(repMarkClustersKernel, dim3(flatGrid(n, ctx->numCU)), dim3(256), 0, ctx->stream, cl->d_repOf.as<uint32_t>(), n, dMark.as<uint32_t>());
    return gatherMarked(ctx, what, db, dMark.as<uint32_t>(), out);
}

extern "C" int plasship_merged_repseqs(plasship_ctx *ctx, const plasship_merged *m, const plasship_seqdb *db, plasship_seqdb **out) {
    const char *what = "plasship_merged_repseqs";
    if (!ctx || !m || !db || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (const int rc = refuseForeign(what, m, db)) return rc;
    if (const int rc = refuseWideIds(what, db)) return rc;
    PH_ENTER(ctx);
    const uint32_t n = (uint32_t) db->n;
    DevBuf dMark, dBad;
    if (dMark.alloc(std::max<size_t>(n, 1) * 4) != hipSuccess || dBad.alloc(8) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(hipMemsetAsync(dMark.p, 0, std::max<size_t>(n, 1) * 4, ctx->stream));
    PH_CHECK(hipMemsetAsync(dBad.p, 0, 8, ctx->stream));
    if (n) hipLaunchKernelGGL(repMarkMergedKernel, dim3(flatGrid(n, ctx->numCU)), dim3(256), 0, ctx->stream, m->d_pairs.as<uint64_t>(), n, dMark.as<uint32_t>(), dBad.as<unsigned long long>());
    unsigned long long hb = 0;
    PH_CHECK(hipMemcpyAsync(&hb, dBad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    if (hb) { setError(std::string(what) + ": the merged clustering names an id outside the DB"); return PLASSHIP_ERR_ARG; }
    return gatherMarked(ctx, what, db, dMark.as<uint32_t>(), out);
}
