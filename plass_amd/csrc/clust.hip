// plasship: clust --cluster-mode 2 | 3 (greedy incremental clustering, low-memory variant) and linclust's pre-cluster subset, on gfx950.
// Product code, built into the extension library libplasship_clust.so (include/plasship_ext/clust.h).  This is the `clust` call of lib/mmseqs/data/workflow/linclust.sh:35,82 as `penguin guided_nuclassemble` makes it
// (--cov-mode 1 -> GREEDY_MEM, workflow/Linclust.cpp:67-76), and what linclust.sh:39-56 leaves of `pref` behind it.
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   commons/DBReader.cpp:298-315, DBReader.h:367-379   SORT_BY_LENGTH: ids in the order of the .index length column descending, ties by
//                                                      the position in key order ascending (comparePairBySeqLength) — the RANK below
//   clustering/ClusteringAlgorithms.cpp:17-23          the result DB must have as many entries as the sequence DB
//   clustering/ClusteringAlgorithms.cpp:271-320        greedyIncrementalLowMem, pass 1: every query lowers assigned[] of itself and of
//                                                      every target it lists to its own rank (a compare-and-swap loop: a minimum)
//   clustering/ClusteringAlgorithms.cpp:322-330        pass 2, the correction loop (see below)
//   clustering/ClusteringAlgorithms.cpp:127-145        (key of the representative, key of the member), sorted as pairs
//   clustering/Clustering.cpp:85-114                   writeData: one entry per representative: its own key, then the other members ascending
//   util/createsubdb.cpp, util/filterdb.cpp:389-410    linclust.sh:39-56: the entries of `pref` whose query is a representative, and in
//                                                      them the lines whose first column is one (a positive filter on column 1)
//
// PASS 2 IS ORDER-FREE.  The reference walks id = 0 .. n-1 and, with a = assigned[id], sets assigned[a] = a when assigned[a] != a.  assigned[y] <= y
// holds from the start (assigned[y] = y, then only lowered, or set back to y), so iteration y writes slot a = assigned[y] <= y, and a == y
// writes nothing new: a slot x is only ever changed by an iteration y > x.  Iteration y therefore reads assigned[y] as pass 1 left it
// (assigned0[y]), and slot x ends as x exactly when assigned0[x] != x and some y has assigned0[y] == x; every other slot keeps assigned0.
// Two kernels over the snapshot assigned0 — flag, then apply into a second array — compute that; nothing is updated in place.
//
// Kernel design: the rank comes from one device radix sort of (~length << 32 | id).  Pass 1 is ONE WAVEFRONT per query, a lane per line and
// step (the line's target id, one atomicMin on assigned[rank[target]]); a query with more than CL_WAVE_MAX_LINES lines (edge lists are
// skewed: one long contig may list thousands of targets) is put on a list and taken by a whole workgroup in a second launch.  Self edges,
// duplicate lines and the unscored identity stubs of an alignment list are minima that change nothing.  The pairs are sorted by a second
// radix sort (ids are ranks in key order, so id order is key order) and the entries' text is laid out by a scan of the per-pair byte counts.
// Algorithmic bytes: 16 per sequence and sort pass, 4 (target id) + one 4-byte atomic per edge; unmeasured, see DESIGN.md.
//
// This file also defines what clust_shared.hpp declares for the whole clustering family (clust_cc.hip, merge_clusters.hip, repseqs.hip): the
// length rank, the key sort, the list-against-DB checks, and count, download and the cluster-DB writer of a PairList.
#include "clust_shared.hpp"
#include "../../include/plasship_ext/clust.h"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <rocprim/device/device_radix_sort.hpp>
#include <algorithm>
#include <cstring>
#include <memory>

namespace plasship {

constexpr int CL_BLOCK = 256;
constexpr uint32_t CL_WAVE_MAX_LINES = 1024;     // 16 steps of a wavefront; longer lists go to the workgroup kernel

__global__ void lengthRankKeyKernel(const uint32_t *__restrict__ len, uint64_t *__restrict__ keys, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = ((uint64_t) ~len[i] << 32) | i;
}
__global__ void clustRankScatterKernel(const uint64_t *__restrict__ sorted, uint32_t *__restrict__ rank, uint32_t *__restrict__ idOfRank,
                                       uint32_t *__restrict__ assigned, uint32_t n) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t id = (uint32_t) sorted[r];
        rank[id] = r; idOfRank[r] = id; assigned[r] = r;
    }
}

// stats: [0] queries on the long list, [1] lines that name an id outside the DB, [2] representatives, [3] promoted by pass 2
template <class Rec>
__device__ __forceinline__ unsigned edgesOfQuery(const Rec *__restrict__ recs, uint64_t b, uint64_t e, unsigned first, unsigned step, uint32_t n, uint32_t rq,
                                                 const uint32_t *__restrict__ rank, uint32_t *__restrict__ assigned) {
    unsigned bad = 0;
    for (uint64_t i = b + first; i < e; i += step) {
        uint32_t q, t;
        if (!lineOf(recs[i], q, t)) continue;
        if (t >= n) { bad++; continue; }
        atomicMin(&assigned[rank[t]], rq);
    }
    return bad;
}
template <class Rec>
__global__ __launch_bounds__(CL_BLOCK) void clustEdgeWaveKernel(const uint64_t *__restrict__ qoff, const Rec *__restrict__ recs, uint32_t n, const uint32_t *__restrict__ rank,
                                                                uint32_t *__restrict__ assigned, uint32_t *__restrict__ longList, uint32_t longCap, unsigned long long *stats) {
    const unsigned lane = (unsigned) laneId();
    const uint64_t wavesPerBlock = CL_BLOCK / WAVE, stride = (uint64_t) gridDim.x * wavesPerBlock;
    unsigned bad = 0;
    for (uint64_t q = (uint64_t) blockIdx.x * wavesPerBlock + threadIdx.x / WAVE; q < n; q += stride) {
        const uint64_t b = qoff[q], e = qoff[q + 1];
        if (e <= b) continue;
        if (e - b > CL_WAVE_MAX_LINES) {
            if (lane == 0) { const unsigned long long slot = atomicAdd(&stats[0], 1ull); if (slot < longCap) longList[slot] = (uint32_t) q; }
            continue;
        }
        bad += edgesOfQuery(recs, b, e, lane, WAVE, n, rank[q], rank, assigned);
    }
    if (bad) atomicAdd(&stats[1], (unsigned long long) bad);
}
template <class Rec>
__global__ __launch_bounds__(CL_BLOCK) void clustEdgeBlockKernel(const uint64_t *__restrict__ qoff, const Rec *__restrict__ recs, uint32_t n, const uint32_t *__restrict__ rank,
                                                                 uint32_t *__restrict__ assigned, const uint32_t *__restrict__ longList, uint32_t longCap, unsigned long long *stats) {
    const unsigned long long nLong = stats[0] < longCap ? stats[0] : longCap;      // (written by the launch before this one)
    unsigned bad = 0;
    for (unsigned long long k = blockIdx.x; k < nLong; k += gridDim.x) {
        const uint32_t q = longList[k];
        bad += edgesOfQuery(recs, qoff[q], qoff[q + 1], threadIdx.x, CL_BLOCK, n, rank[q], rank, assigned);
    }
    if (bad) atomicAdd(&stats[1], (unsigned long long) bad);
}

// pass 2 over the snapshot: flag[x] = 1 when x is named by some y and is not its own representative ...
__global__ void clustFlagKernel(const uint32_t *__restrict__ assigned0, uint32_t *__restrict__ flag, uint32_t n) {
    for (uint32_t y = blockIdx.x * blockDim.x + threadIdx.x; y < n; y += gridDim.x * blockDim.x) {
        const uint32_t x = assigned0[y];                 // (< n: a rank)
        if (assigned0[x] != x) flag[x] = 1u;             // (every writer stores the same value)
    }
}
// ... and the result, per id: the representative's id, and the pair (representative id << 32 | member id)
__global__ void clustApplyKernel(const uint32_t *__restrict__ assigned0, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                 const uint32_t *__restrict__ idOfRank, uint32_t *__restrict__ repOf, uint64_t *__restrict__ pairs, uint32_t n, unsigned long long *stats) {
    int reps = 0, promoted = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t r = rank[i];
        const bool up = flag[r] != 0;
        const uint32_t rep = idOfRank[up ? r : assigned0[r]];
        repOf[i] = rep; pairs[i] = ((uint64_t) rep << 32) | i;
        reps += rep == i; promoted += up;
    }
    reps = waveReduceSum(reps); promoted = waveReduceSum(promoted);
    if (laneId() == 0) { if (reps) atomicAdd(&stats[2], (unsigned long long) reps); if (promoted) atomicAdd(&stats[3], (unsigned long long) promoted); }
}

// ---- the cluster DB's text: pair j contributes the entry's '\0' when it closes one and, before it, its member's line.  repFirst
//      (Clustering::writeData): the representative's line when it opens an entry, and no member line when it is the representative ----
__device__ __forceinline__ uint32_t decDigits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ char *putKeyLine(char *p, uint32_t v) {
    const uint32_t d = decDigits(v);
    for (uint32_t k = d; k > 0; k--) { p[k - 1] = (char) ('0' + v % 10u); v /= 10u; }
    p[d] = '\n';
    return p + d + 1;
}
__device__ __forceinline__ void pairEnds(const uint64_t *__restrict__ pairs, uint64_t j, uint64_t n, bool &head, bool &tail) {
    const uint32_t rep = (uint32_t) (pairs[j] >> 32);
    head = j == 0 || (uint32_t) (pairs[j - 1] >> 32) != rep;
    tail = j + 1 == n || (uint32_t) (pairs[j + 1] >> 32) != rep;
}
template <bool repFirst>
__global__ void pairTextLenKernel(const uint64_t *__restrict__ pairs, const uint32_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ bytes, uint32_t *__restrict__ heads) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t rep = (uint32_t) (pairs[j] >> 32), mem = (uint32_t) pairs[j];
        bool head, tail; pairEnds(pairs, j, n, head, tail);
        bytes[j] = (repFirst && head ? decDigits(keys[rep]) + 1u : 0u) + (!repFirst || mem != rep ? decDigits(keys[mem]) + 1u : 0u) + (tail ? 1u : 0u);
        heads[j] = head ? 1u : 0u;
    }
}
template <bool repFirst>
__global__ void pairTextWriteKernel(const uint64_t *__restrict__ pairs, const uint32_t *__restrict__ keys, uint64_t n, const uint64_t *__restrict__ pos,
                                    const uint64_t *__restrict__ entryOf, char *__restrict__ text, uint64_t *__restrict__ entryOff, uint32_t *__restrict__ entryKey) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t rep = (uint32_t) (pairs[j] >> 32), mem = (uint32_t) pairs[j];
        bool head, tail; pairEnds(pairs, j, n, head, tail);
        char *p = text + pos[j];                          // (pos[j + 1] - pos[j] bytes are this pair's: pairTextLenKernel counted what is written here)
        if (head) { if (repFirst) p = putKeyLine(p, keys[rep]); entryOff[entryOf[j]] = pos[j]; entryKey[entryOf[j]] = keys[rep]; }
        if (!repFirst || mem != rep) p = putKeyLine(p, keys[mem]);
        if (tail) *p = '\0';
    }
}

// ---- linclust.sh:39-56 on a candidate list: the lines of the representatives' entries whose target is a representative, in input order ----
__global__ void clustFilterFlagKernel(const CandHit *__restrict__ hits, uint64_t nHits, const uint32_t *__restrict__ repOf, uint32_t n, uint32_t *__restrict__ keep,
                                      unsigned long long *stats) {      // stats: [0] kept, [1] kept that are not an implicit self line, [2] ids outside the DB
    int kept = 0, visible = 0, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nHits; i += (uint64_t) gridDim.x * blockDim.x) {
        const CandHit h = hits[i];
        bool k = false;
        if (h.query >= n || h.target >= n) bad++;
        else k = repOf[h.query] == h.query && repOf[h.target] == h.target;
        keep[i] = k ? 1u : 0u;
        kept += k; visible += k && !(h.query == h.target && h.prefScore == 0 && h.diag16 == 0);
    }
    kept = waveReduceSum(kept); visible = waveReduceSum(visible); bad = waveReduceSum(bad);
    if (laneId() == 0) {
        if (kept) atomicAdd(&stats[0], (unsigned long long) kept);
        if (visible) atomicAdd(&stats[1], (unsigned long long) visible);
        if (bad) atomicAdd(&stats[2], (unsigned long long) bad);
    }
}

int sortKeysU64(plasship_ctx *ctx, const char *what, uint64_t *in, uint64_t *out, uint64_t n) {
    if (n > 0xFFFFFFFFull) { setError(std::string(what) + ": list sizes are 32-bit"); return PLASSHIP_ERR_UNSUPPORTED; }      // (rocPRIM's size; every caller refuses earlier, at its own limit)
    size_t tmpBytes = 0;
    PH_CHECK(rocprim::radix_sort_keys(nullptr, tmpBytes, in, out, (unsigned int) n, 0, 64, ctx->stream));
    DevBuf tmp;
    if (tmp.alloc(std::max<size_t>(tmpBytes, 8)) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
    PH_CHECK(rocprim::radix_sort_keys(tmp.p, tmpBytes, in, out, (unsigned int) n, 0, 64, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));          // (tmp is released with this function)
    return PLASSHIP_OK;
}
int lengthRank(plasship_ctx *ctx, const char *what, const plasship_seqdb *db, uint64_t *keysTmp, uint64_t *sortedOut) {
    hipLaunchKernelGGL(lengthRankKeyKernel, dim3(flatGrid(db->n, ctx->numCU)), dim3(256), 0, ctx->stream, db->d_len.as<uint32_t>(), keysTmp, (uint32_t) db->n);
    return sortKeysU64(ctx, what, keysTmp, sortedOut, db->n);
}

template <class Rec>
static int clustGreedy(plasship_ctx *ctx, const plasship_seqdb *db, const uint64_t *dQoff, const Rec *dRecs, uint64_t nRecs, plasship_clusters **out,
                       plasship_clust_stats *stats, const char *what) {
    PH_ENTER(ctx);
    if (const int rc = refuseWideIds(what, db)) return rc;
    const uint32_t n = (uint32_t) db->n;
    const uint64_t n1 = std::max<uint32_t>(n, 1);
    const uint32_t longCap = (uint32_t) std::min<uint64_t>(n1, nRecs / (CL_WAVE_MAX_LINES + 1) + 1);
    std::unique_ptr<plasship_clusters> holder(new plasship_clusters());     // released to the caller on success only
    plasship_clusters *cl = holder.get();
    cl->n = n; cl->dbGen = db->gen;
    DevBuf dKeys, dSorted, dRank, dIdOfRank, dAssigned, dFlag, dLong, dStats, dPairs;
    if (dKeys.alloc(n1 * 8) != hipSuccess || dSorted.alloc(n1 * 8) != hipSuccess || dRank.alloc(n1 * 4) != hipSuccess || dIdOfRank.alloc(n1 * 4) != hipSuccess ||
        dAssigned.alloc(n1 * 4) != hipSuccess || dFlag.alloc(n1 * 4) != hipSuccess || dLong.alloc((uint64_t) longCap * 4) != hipSuccess || dStats.alloc(32) != hipSuccess ||
        dPairs.alloc(n1 * 8) != hipSuccess || cl->d_pairs.alloc(n1 * 8) != hipSuccess || cl->d_repOf.alloc(n1 * 4) != hipSuccess) {
        setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    unsigned long long hs[4] = {0, 0, 0, 0};
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 32, ctx->stream));
    PH_CHECK(hipMemsetAsync(dFlag.p, 0, n1 * 4, ctx->stream));
    PH_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (n) {
        const unsigned g = flatGrid(n, ctx->numCU);
        // the rank: position in the order (length descending, id ascending)
        if (const int rc = lengthRank(ctx, what, db, dKeys.as<uint64_t>(), dSorted.as<uint64_t>())) return rc;
        hipLaunchKernelGGL(clustRankScatterKernel, dim3(g), dim3(256), 0, ctx->stream, dSorted.as<uint64_t>(), dRank.as<uint32_t>(), dIdOfRank.as<uint32_t>(), dAssigned.as<uint32_t>(), n);
        // pass 1
        if (nRecs) {
            const unsigned gw = (unsigned) std::min<uint64_t>(((uint64_t) n + CL_BLOCK / WAVE - 1) / (CL_BLOCK / WAVE), (uint64_t) ctx->numCU * 8);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(clustEdgeWaveKernel<Rec>), dim3(gw), dim3(CL_BLOCK), 0, ctx->stream, dQoff, dRecs, n, dRank.as<uint32_t>(), dAssigned.as<uint32_t>(),
                               dLong.as<uint32_t>(), longCap, dStats.as<unsigned long long>());
            hipLaunchKernelGGL(HIP_KERNEL_NAME(clustEdgeBlockKernel<Rec>), dim3((unsigned) std::min<uint64_t>(longCap, (uint64_t) ctx->numCU * 8)), dim3(CL_BLOCK), 0, ctx->stream, dQoff, dRecs, n,
                               dRank.as<uint32_t>(), dAssigned.as<uint32_t>(), dLong.as<uint32_t>(), longCap, dStats.as<unsigned long long>());
        }
        // pass 2, on the snapshot
        hipLaunchKernelGGL(clustFlagKernel, dim3(g), dim3(256), 0, ctx->stream, dAssigned.as<uint32_t>(), dFlag.as<uint32_t>(), n);
        hipLaunchKernelGGL(clustApplyKernel, dim3(g), dim3(256), 0, ctx->stream, dAssigned.as<uint32_t>(), dFlag.as<uint32_t>(), dRank.as<uint32_t>(), dIdOfRank.as<uint32_t>(),
                           cl->d_repOf.as<uint32_t>(), dPairs.as<uint64_t>(), n, dStats.as<unsigned long long>());
        if (const int rc = sortKeysU64(ctx, what, dPairs.as<uint64_t>(), cl->d_pairs.as<uint64_t>(), n)) return rc;
    }
    PH_CHECK(hipEventRecord(ctx->ev[1], ctx->stream));
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hs[1]) { setError(std::string(what) + ": the list names sequences that are not in the DB"); return PLASSHIP_ERR_ARG; }
    cl->nClusters = hs[2];
    if (stats) {
        stats->n_sequences = n; stats->n_edges = nRecs; stats->n_clusters = hs[2]; stats->n_promoted = hs[3]; stats->n_long_queries = hs[0];
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); stats->ms_kernel = ms;
    }
    *out = holder.release();
    return PLASSHIP_OK;
}

int checkListOnDb(const char *what, const plasship_seqdb *db, const plasship_cands *c) {
    if (c->nQueries != db->n) { setError(std::string(what) + ": the candidate list has another number of queries than the DB has sequences"); return PLASSHIP_ERR_ARG; }
    return PLASSHIP_OK;
}
int checkListOnDb(const char *what, const plasship_seqdb *db, const plasship_alns *a) {
    if (a->nQueries != db->n) { setError(std::string(what) + ": the alignment list has another number of queries than the DB has sequences"); return PLASSHIP_ERR_ARG; }
    if (a->qdb != db || a->tdb != db) { setError(std::string(what) + ": the alignment list was built on another DB"); return PLASSHIP_ERR_ARG; }
    return PLASSHIP_OK;
}

int pairListCount(const char *what, const PairList *list, uint64_t *nMembers, uint64_t *nClusters) {
    if (!list) { setError(std::string(what) + ": NULL"); return PLASSHIP_ERR_ARG; }
    if (nMembers) *nMembers = list->n;
    if (nClusters) *nClusters = list->nClusters;
    return PLASSHIP_OK;
}

int pairListDownload(plasship_ctx *ctx, const char *what, const PairList *list, const plasship_seqdb *db, uint32_t *repKey, uint32_t *memberKey) {
    if (!ctx || !list || !db) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseForeign(what, list, db)) return rc;
    PH_ENTER(ctx);
    const size_t n = list->n;
    std::vector<uint32_t> keys(n); std::vector<uint64_t> pairs(n);
    PH_CHECK(plasship::streamSync(ctx->stream));
    if (n) {
        int rc = stagedCopyToHost(ctx, keys.data(), db->d_key.p, n * 4); if (rc) return rc;
        rc = stagedCopyToHost(ctx, pairs.data(), list->d_pairs.p, n * 8); if (rc) return rc;
    }
    for (size_t j = 0; j < n; j++) {
        if (repKey) repKey[j] = keys[(size_t) (pairs[j] >> 32)];
        if (memberKey) memberKey[j] = keys[(size_t) (uint32_t) pairs[j]];
    }
    return PLASSHIP_OK;
}

int pairListWrite(plasship_ctx *ctx, const char *what, const PairList *list, const plasship_seqdb *db, const char *dbPath, bool repFirst) {
    if (!ctx || !list || !db || !dbPath) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseForeign(what, list, db)) return rc;
    PH_ENTER(ctx);
    const uint64_t n = list->n, nC = list->nClusters;
    std::vector<uint64_t> entryOff(nC + 1, 0); std::vector<uint32_t> entryKey(nC), elen(nC);
    uint64_t total = 0;
    DevBuf dBytes, dHeads, dPos, dEntryOf, dTmp, dText, dEntryOff, dEntryKey;
    if (n) {
        const size_t tmpBytes = exclusiveScanTmpBytes(n);
        if (dBytes.alloc(n * 4) != hipSuccess || dHeads.alloc(n * 4) != hipSuccess || dPos.alloc((n + 1) * 8) != hipSuccess || dEntryOf.alloc((n + 1) * 8) != hipSuccess ||
            dTmp.alloc(tmpBytes) != hipSuccess || dEntryOff.alloc(std::max<uint64_t>(nC, 1) * 8) != hipSuccess || dEntryKey.alloc(std::max<uint64_t>(nC, 1) * 4) != hipSuccess) {
            setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
        }
        const unsigned g = flatGrid(n, ctx->numCU);
        hipLaunchKernelGGL(repFirst ? pairTextLenKernel<true> : pairTextLenKernel<false>, dim3(g), dim3(256), 0, ctx->stream, list->d_pairs.as<uint64_t>(), db->d_key.as<uint32_t>(), n,
                           dBytes.as<uint32_t>(), dHeads.as<uint32_t>());
        if (exclusiveScanU32(ctx->stream, dBytes.as<uint32_t>(), dPos.as<uint64_t>(), n, dTmp.p, tmpBytes) ||
            exclusiveScanU32(ctx->stream, dHeads.as<uint32_t>(), dEntryOf.as<uint64_t>(), n, dTmp.p, tmpBytes)) { (void) plasship::streamSync(ctx->stream); setError("scan failed"); return PLASSHIP_ERR_DEVICE; }
        uint64_t ends[2] = {0, 0};
        PH_CHECK(hipMemcpyAsync(&ends[0], dPos.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_CHECK(hipMemcpyAsync(&ends[1], dEntryOf.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        PH_CHECK(plasship::streamSync(ctx->stream));
        total = ends[0];
        if (ends[1] != nC) { setError(std::string(what) + ": internal error: the number of entries differs from the number of clusters"); return PLASSHIP_ERR_DEVICE; }
        if (dText.alloc(std::max<uint64_t>(total, 1)) != hipSuccess) { setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE; }
        hipLaunchKernelGGL(repFirst ? pairTextWriteKernel<true> : pairTextWriteKernel<false>, dim3(g), dim3(256), 0, ctx->stream, list->d_pairs.as<uint64_t>(), db->d_key.as<uint32_t>(), n,
                           dPos.as<uint64_t>(), dEntryOf.as<uint64_t>(), dText.as<char>(), dEntryOff.as<uint64_t>(), dEntryKey.as<uint32_t>());
        PH_CHECK(plasship::streamSync(ctx->stream));
        PH_CHECK(hipGetLastError());
        int rc = stagedCopyToHost(ctx, entryOff.data(), dEntryOff.p, nC * 8); if (rc) return rc;
        rc = stagedCopyToHost(ctx, entryKey.data(), dEntryKey.p, nC * 4); if (rc) return rc;
    }
    entryOff[nC] = total;
    for (uint64_t c = 0; c < nC; c++) elen[c] = (uint32_t) (entryOff[c + 1] - entryOff[c]);
    DBFileWriter w; std::string err;
    if (!w.open(dbPath, PLASSHIP_DBTYPE_CLUSTER_RES, err)) { setError(err); return PLASSHIP_ERR_IO; }
    if (total) {
        const int rc = stagedDownload(ctx, dText.p, total, [&](const char *src, uint64_t, uint64_t bytes) { w.data(src, bytes); return !w.failed.load(); });
        if (rc) { setError(std::string(what) + ": writing " + dbPath + " failed"); return rc; }
    }
    w.index(entryKey.data(), elen.data(), nC);
    if (!w.close(err)) { setError(err); return PLASSHIP_ERR_IO; }
    return PLASSHIP_OK;
}

}  // namespace plasship
using namespace plasship;

extern "C" int plasship_clust_greedy_cands(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, plasship_clusters **out, plasship_clust_stats *stats) {
    const char *what = "plasship_clust_greedy_cands";
    if (!ctx || !db || !c || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (const int rc = checkListOnDb(what, db, c)) return rc;
    return clustGreedy<CandHit>(ctx, db, c->d_qoff.as<uint64_t>(), c->d_hits.as<CandHit>(), c->nHits, out, stats, what);
}

extern "C" int plasship_clust_greedy_alns(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_alns *a, plasship_clusters **out, plasship_clust_stats *stats) {
    const char *what = "plasship_clust_greedy_alns";
    if (!ctx || !db || !a || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (const int rc = checkListOnDb(what, db, a)) return rc;
    return clustGreedy<AlnRec>(ctx, db, a->d_qoff.as<uint64_t>(), a->d_recs.as<AlnRec>(), a->nSlots, out, stats, what);
}

extern "C" int plasship_clusters_count(const plasship_clusters *cl, uint64_t *n_members, uint64_t *n_clusters) {
    return pairListCount("plasship_clusters_count", cl, n_members, n_clusters);
}

extern "C" void plasship_clusters_free(plasship_ctx *ctx, plasship_clusters *cl) {
    if (!cl) return;
    if (ctx) { (void) hipSetDevice(ctx->device); plasship::poolEnter(ctx->stream); }
    delete cl;
}

extern "C" int plasship_clusters_download(plasship_ctx *ctx, const plasship_clusters *cl, const plasship_seqdb *db, uint32_t *rep_key, uint32_t *member_key) {
    return pairListDownload(ctx, "plasship_clusters_download", cl, db, rep_key, member_key);
}

extern "C" int plasship_clusters_write(plasship_ctx *ctx, const plasship_clusters *cl, const plasship_seqdb *db, const char *db_path) {
    return pairListWrite(ctx, "plasship_clusters_write", cl, db, db_path, true);
}

extern "C" int plasship_cands_filter(plasship_ctx *ctx, const plasship_cands *c, const plasship_clusters *cl, plasship_cands **out) {
    const char *what = "plasship_cands_filter";
    if (!ctx || !c || !cl || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (c->nQueries != cl->n) { setError(std::string(what) + ": the candidate list and the clustering belong to DBs of different sizes"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    const uint64_t nHits = c->nHits; const size_t nQ = c->nQueries;
    DevBuf dKeep, dStats;
    if (dKeep.alloc(std::max<uint64_t>(nHits, 1) * 4) != hipSuccess || dStats.alloc(32) != hipSuccess) {
        setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 32, ctx->stream));
    if (nHits) hipLaunchKernelGGL(clustFilterFlagKernel, dim3(flatGrid(nHits, ctx->numCU)), dim3(256), 0, ctx->stream, c->d_hits.as<CandHit>(), nHits, cl->d_repOf.as<uint32_t>(), (uint32_t) cl->n,
                                  dKeep.as<uint32_t>(), dStats.as<unsigned long long>());
    unsigned long long hs[4] = {0, 0, 0, 0};
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hs[2]) { setError(std::string(what) + ": the candidate list names sequences that are not in the clustered DB"); return PLASSHIP_ERR_ARG; }
    std::unique_ptr<plasship_cands> holder(new plasship_cands());     // released to the caller on success only
    plasship_cands *o = holder.get();
    o->reverseCapable = c->reverseCapable; o->nQueries = nQ; o->nHits = hs[0]; o->nNonSelf = hs[1];
    if (const int rc = compactCsr(ctx, what, c->d_qoff.as<uint64_t>(), nQ, c->d_hits.p, sizeof(CandHit), dKeep.as<uint32_t>(), nHits, hs[0], o->d_qoff, o->d_hits)) return rc;
    // the entries that are left: the representatives' (createsubdb --subdb-mode 1 with pre_clust's keys); plasship_cands_write writes these only
    std::vector<uint32_t> repOf(nQ);
    if (nQ) { const int rc = stagedCopyToHost(ctx, repOf.data(), cl->d_repOf.p, nQ * 4); if (rc) return rc; }
    o->h_present.resize(nQ);
    for (size_t q = 0; q < nQ; q++) o->h_present[q] = repOf[q] == q ? 1 : 0;
    *out = holder.release();
    return PLASSHIP_OK;
}
