// plasship: mergeclusters for two clusterings of one sequence DB, on gfx950.  Product code, built into the extension library
// libplasship_linclust.so (include/plasship_ext/linclust.h).  This is the last call of lib/mmseqs/data/workflow/linclust.sh (line 87):
// pre_clust (made on the sequence DB) and clust (made on the subset DB of pre_clust's representatives, keys preserved) become the
// workflow's result.
//
// Reference behaviour reproduced (lib/mmseqs/src/util/mergeclusters.cpp):
//   :28-64    every entry of the first clustering is a list (in the entry's line order) under its representative
//   :66-107   every entry R of the second clustering: the list of each member other than R is spliced behind R's list, in the entry's
//             line order; R's own list stays where it is, in front
//   :125-146  the writer walks the sequence DB in key order and SKIPS a sequence whose list is empty: it gets no entry
// With the entries laid out as Clustering::writeData writes them (own key first, the others ascending) the place of sequence x in the
// merged DB is a sum of three offsets, no list is ever built: with r = first representative of x and R = second representative of r,
//   place(x) = [members of the clusters before R]  +  [sizes of R's second-step members before r: R's own list first, the others ascending]
//            + [x's place in r's list: r first, the others ascending]
// Both clusterings are sorted pair arrays (representative id << 32 | member id; ids are ranks in key order), so the first term and the
// second are differences of ONE exclusive scan of the first-step cluster sizes taken in the second clustering's pair order, and the third
// is x's index in its segment.  Three flat kernels and a scan; the merged DB is written by the family's one writer (pairListWrite, clust_shared.hpp).
// Every index is bounds-checked against n before it is used: a clustering that names an id outside the DB ends with an error.
// Algorithmic bytes: 8 (pair) + ~28 (the per-id arrays) read and 8 written per sequence, twice 12 for the scans; unmeasured, see DESIGN.md.
#include "clust_shared.hpp"
#include "../../include/plasship_ext/linclust.h"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <cstring>
#include <memory>

namespace plasship {

// [0] = ids outside the DB, [1] = places outside [0, n)
__global__ void mergeSegKernel(const uint64_t *__restrict__ p1, uint32_t n, uint32_t *__restrict__ start1, uint32_t *__restrict__ end1, unsigned long long *bad) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t rep = (uint32_t) (p1[j] >> 32), mem = (uint32_t) p1[j];
        if (rep >= n || mem >= n) { atomicAdd(&bad[0], 1ull); continue; }
        if (j == 0 || (uint32_t) (p1[j - 1] >> 32) != rep) start1[rep] = (uint32_t) j;
        if (j + 1 == n || (uint32_t) (p1[j + 1] >> 32) != rep) end1[rep] = (uint32_t) j + 1u;
    }
}
// the size of a sequence's first-step list: 0 unless it is a representative there
__device__ __forceinline__ uint32_t listSize(const uint32_t *repOf1, const uint32_t *start1, const uint32_t *end1, uint32_t m) { return repOf1[m] == m ? end1[m] - start1[m] : 0u; }
__global__ void mergeSizeKernel(const uint64_t *__restrict__ p2, uint32_t n, const uint32_t *__restrict__ repOf1, const uint32_t *__restrict__ start1,
                                const uint32_t *__restrict__ end1, uint32_t *__restrict__ val, uint32_t *__restrict__ start2, uint32_t *__restrict__ pos2, unsigned long long *bad) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t rep = (uint32_t) (p2[j] >> 32), mem = (uint32_t) p2[j];
        if (rep >= n || mem >= n) { atomicAdd(&bad[0], 1ull); val[j] = 0; continue; }
        val[j] = listSize(repOf1, start1, end1, mem);
        pos2[mem] = (uint32_t) j;
        if (j == 0 || (uint32_t) (p2[j - 1] >> 32) != rep) start2[rep] = (uint32_t) j;
    }
}
__global__ void mergePlaceKernel(const uint64_t *__restrict__ p1, uint32_t n, const uint32_t *__restrict__ repOf1, const uint32_t *__restrict__ start1,
                                 const uint32_t *__restrict__ end1, const uint32_t *__restrict__ repOf2, const uint32_t *__restrict__ start2, const uint32_t *__restrict__ pos2,
                                 const uint64_t *__restrict__ S, uint64_t *__restrict__ out, unsigned long long *bad) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t) (p1[j] >> 32), x = (uint32_t) p1[j];
        if (r >= n || x >= n) continue;                       // (counted by mergeSegKernel)
        const uint32_t R = repOf2[r];
        if (R >= n) { atomicAdd(&bad[0], 1ull); continue; }
        const uint32_t s2 = start2[R], jr = pos2[r];
        if (s2 >= n || jr >= n || jr < s2) { atomicAdd(&bad[1], 1ull); continue; }
        const uint64_t group = r == R ? 0ull : (S[jr] - S[s2]) + (r < R ? (uint64_t) listSize(repOf1, start1, end1, R) : 0ull);
        const uint64_t within = x == r ? 0ull : (j - start1[r]) + (x < r ? 1ull : 0ull);
        const uint64_t place = S[s2] + group + within;
        if (place >= n) { atomicAdd(&bad[1], 1ull); continue; }
        out[place] = (uint64_t) R << 32 | x;
    }
}

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_clusters_merge(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_clusters *first, const plasship_clusters *second, plasship_merged **out) {
    const char *what = "plasship_clusters_merge";
    if (!ctx || !db || !first || !second || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (first->n != db->n || first->dbGen != db->gen || second->n != db->n || second->dbGen != db->gen) {
        setError(std::string(what) + ": a clustering does not belong to this DB (a clustering of a subset DB comes in through plasship_clusters_read, by key)"); return PLASSHIP_ERR_ARG;
    }
    if (const int rc = refuseWideIds(what, db)) return rc;
    PH_ENTER(ctx);
    const uint32_t n = (uint32_t) db->n;
    std::unique_ptr<plasship_merged> holder(new plasship_merged());     // released to the caller on success only
    plasship_merged *m = holder.get();
    m->n = n; m->dbGen = db->gen;
    if (n == 0) { *out = holder.release(); return PLASSHIP_OK; }
    const size_t tmpBytes = exclusiveScanTmpBytes(n);
    DevBuf dStart1, dEnd1, dVal, dStart2, dPos2, dS, dTmp, dBad;
    if (dStart1.alloc((size_t) n * 4) != hipSuccess || dEnd1.alloc((size_t) n * 4) != hipSuccess || dVal.alloc((size_t) n * 4) != hipSuccess || dStart2.alloc((size_t) n * 4) != hipSuccess ||
        dPos2.alloc((size_t) n * 4) != hipSuccess || dS.alloc(((size_t) n + 1) * 8) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess || dBad.alloc(16) != hipSuccess ||
        m->d_pairs.alloc((size_t) n * 8) != hipSuccess) {
        setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dBad.p, 0, 16, ctx->stream));
    PH_CHECK(hipMemsetAsync(dStart1.p, 0, (size_t) n * 4, ctx->stream));
    PH_CHECK(hipMemsetAsync(dEnd1.p, 0, (size_t) n * 4, ctx->stream));
    PH_CHECK(hipMemsetAsync(dStart2.p, 0xFF, (size_t) n * 4, ctx->stream));      // (no segment: caught by the bounds check)
    PH_CHECK(hipMemsetAsync(dPos2.p, 0xFF, (size_t) n * 4, ctx->stream));
    PH_CHECK(hipMemsetAsync(m->d_pairs.p, 0xFF, (size_t) n * 8, ctx->stream));   // (a place nobody takes stays recognisable)
    const unsigned g = flatGrid(n, ctx->numCU);
    unsigned long long *bad = dBad.as<unsigned long long>();
    hipLaunchKernelGGL(mergeSegKernel, dim3(g), dim3(256), 0, ctx->stream, first->d_pairs.as<uint64_t>(), n, dStart1.as<uint32_t>(), dEnd1.as<uint32_t>(), bad);
    hipLaunchKernelGGL(mergeSizeKernel, dim3(g), dim3(256), 0, ctx->stream, second->d_pairs.as<uint64_t>(), n, first->d_repOf.as<uint32_t>(), dStart1.as<uint32_t>(), dEnd1.as<uint32_t>(),
                       dVal.as<uint32_t>(), dStart2.as<uint32_t>(), dPos2.as<uint32_t>(), bad);
    if (exclusiveScanU32(ctx->stream, dVal.as<uint32_t>(), dS.as<uint64_t>(), n, dTmp.p, tmpBytes)) { (void) plasship::streamSync(ctx->stream); setError(std::string(what) + ": scan failed"); return PLASSHIP_ERR_DEVICE; }
    hipLaunchKernelGGL(mergePlaceKernel, dim3(g), dim3(256), 0, ctx->stream, first->d_pairs.as<uint64_t>(), n, first->d_repOf.as<uint32_t>(), dStart1.as<uint32_t>(), dEnd1.as<uint32_t>(),
                       second->d_repOf.as<uint32_t>(), dStart2.as<uint32_t>(), dPos2.as<uint32_t>(), dS.as<uint64_t>(), m->d_pairs.as<uint64_t>(), bad);
    unsigned long long hb[2] = {0, 0}; uint64_t total = 0;
    PH_CHECK(hipMemcpyAsync(hb, dBad.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(hipMemcpyAsync(&total, dS.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hb[0] || hb[1] || total != n) { setError(std::string(what) + ": the two clusterings do not fit together (an id outside the DB, or a first-step representative the second step lists under two clusters)"); return PLASSHIP_ERR_ARG; }
    // the clusters: the pairs whose representative differs from the one before (on the host: n * 8 bytes once, the caller writes or downloads them anyway)
    std::vector<uint64_t> pairs(n);
    { const int rc = stagedCopyToHost(ctx, pairs.data(), m->d_pairs.p, (uint64_t) n * 8); if (rc) return rc; }
    for (uint32_t j = 0; j < n; j++) {
        if ((pairs[j] >> 32) >= n || (uint32_t) pairs[j] >= n) { setError(std::string(what) + ": internal error: a place of the merged DB was not filled"); return PLASSHIP_ERR_DEVICE; }
        m->nClusters += j == 0 || (pairs[j] >> 32) != (pairs[j - 1] >> 32);
    }
    *out = holder.release();
    return PLASSHIP_OK;
}

extern "C" int plasship_merged_count(const plasship_merged *m, uint64_t *n_members, uint64_t *n_clusters) {
    return pairListCount("plasship_merged_count", m, n_members, n_clusters);
}

extern "C" void plasship_merged_free(plasship_ctx *ctx, plasship_merged *m) {
    if (!m) return;
    if (ctx) { (void) hipSetDevice(ctx->device); plasship::poolEnter(ctx->stream); }
    delete m;
}

extern "C" int plasship_merged_download(plasship_ctx *ctx, const plasship_merged *m, const plasship_seqdb *db, uint32_t *rep_key, uint32_t *member_key) {
    return pairListDownload(ctx, "plasship_merged_download", m, db, rep_key, member_key);
}

extern "C" int plasship_merged_write(plasship_ctx *ctx, const plasship_merged *m, const plasship_seqdb *db, const char *db_path) {
    return pairListWrite(ctx, "plasship_merged_write", m, db, db_path, false);
}

// A cluster DB (dbtype 6) from disk as a clustering of `db`, BY KEY: an entry's key is the representative, its lines are the members.  A
// sequence of `db` no entry lists is a cluster of its own — what a clustering made on a subset DB (linclust's second `clust`, on the
// representatives of the first) says about the sequences outside the subset, as far as mergeclusters reads it.
extern "C" int plasship_clusters_read(plasship_ctx *ctx, const plasship_seqdb *db, const char *db_path, plasship_clusters **out) {
    const char *what = "plasship_clusters_read";
    if (!ctx || !db || !db_path || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseWideIds(what, db)) return rc;
    PH_ENTER(ctx);
    HostDB h; std::string err;
    if (!readDBFiles(db_path, h, err)) { setError(err); return PLASSHIP_ERR_IO; }
    if ((h.dbtype & 0x3FFFFFFF) != PLASSHIP_DBTYPE_CLUSTER_RES) { setError(std::string(what) + ": " + db_path + " is not a cluster DB"); return PLASSHIP_ERR_ARG; }
    const size_t n = db->n;
    std::vector<uint32_t> keys(n);
    PH_CHECK(plasship::streamSync(ctx->stream));
    if (n) { const int rc = stagedCopyToHost(ctx, keys.data(), db->d_key.p, n * 4); if (rc) return rc; }
    auto idOf = [&](uint64_t key, uint32_t &id) {
        const auto it = std::lower_bound(keys.begin(), keys.end(), (uint32_t) key);
        if (key > 0xFFFFFFFFull || it == keys.end() || *it != (uint32_t) key) return false;
        id = (uint32_t) (it - keys.begin()); return true;
    };
    if (!std::is_sorted(keys.begin(), keys.end())) { setError(std::string(what) + ": the sequence DB's ids are not in key order"); return PLASSHIP_ERR_ARG; }
    std::vector<uint32_t> repOf(n);
    std::vector<uint8_t> listed(n, 0);
    for (size_t i = 0; i < n; i++) repOf[i] = (uint32_t) i;
    for (size_t e = 0; e < h.key.size(); e++) {
        uint32_t rep;
        if (!idOf(h.key[e], rep)) { setError(std::string(what) + ": " + db_path + " names key " + std::to_string(h.key[e]) + ", which the sequence DB does not have"); return PLASSHIP_ERR_ARG; }
        if (h.off[e] + h.elen[e] > h.data.size()) { setError(std::string(what) + ": " + db_path + ": an entry lies outside the data file"); return PLASSHIP_ERR_IO; }
        const char *p = h.data.data() + h.off[e], *end = p + h.elen[e];
        while (p < end && *p != '\0') {
            uint64_t key = 0; bool digits = false;
            while (p < end && *p >= '0' && *p <= '9') { key = key * 10 + (uint64_t) (*p - '0'); if (key > 0xFFFFFFFFull) key = 0x100000000ull; digits = true; p++; }
            uint32_t mem;
            if (!digits || !idOf(key, mem)) { setError(std::string(what) + ": " + db_path + ": a line of entry " + std::to_string(h.key[e]) + " is not a key of the sequence DB"); return PLASSHIP_ERR_ARG; }
            if (listed[mem]) { setError(std::string(what) + ": " + db_path + " lists key " + std::to_string(keys[mem]) + " twice"); return PLASSHIP_ERR_ARG; }
            listed[mem] = 1; repOf[mem] = rep;
            while (p < end && *p != '\n' && *p != '\0') p++;
            if (p < end && *p == '\n') p++;
        }
    }
    std::unique_ptr<plasship_clusters> holder(new plasship_clusters());     // released to the caller on success only
    plasship_clusters *cl = holder.get();
    cl->n = n; cl->dbGen = db->gen;
    std::vector<uint64_t> pairs(n);
    for (size_t i = 0; i < n; i++) {
        if (repOf[repOf[i]] != repOf[i]) { setError(std::string(what) + ": " + db_path + ": the representative of key " + std::to_string(keys[i]) + " is listed under another one"); return PLASSHIP_ERR_ARG; }
        pairs[i] = (uint64_t) repOf[i] << 32 | (uint64_t) i;
        cl->nClusters += repOf[i] == i;
    }
    std::sort(pairs.begin(), pairs.end());
    const uint64_t n1 = std::max<size_t>(n, 1);
    if (cl->d_pairs.alloc(n1 * 8) != hipSuccess || cl->d_repOf.alloc(n1 * 4) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
    if (n) {
        int rc = stagedCopyToDevice(ctx, cl->d_pairs.p, pairs.data(), n * 8); if (rc) return rc;
        rc = stagedCopyToDevice(ctx, cl->d_repOf.p, repOf.data(), n * 4); if (rc) return rc;
        PH_CHECK(plasship::streamSync(ctx->stream));
    }
    *out = holder.release();
    return PLASSHIP_OK;
}
