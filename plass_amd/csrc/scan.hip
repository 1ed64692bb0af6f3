// Device-wide exclusive scan (see device_utils.hpp) and what every list filter does with one: compactCsr (common.hpp); the host side of the
// list-in, list-out rescore modules around it: RescoreList (common.hpp).  Product code.
#include "common.hpp"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>

namespace plasship {

template <typename T>
__global__ __launch_bounds__(SCAN_BLOCK) void scanReduceKernel(const T *__restrict__ in, uint64_t *__restrict__ partial, size_t n) {
    __shared__ unsigned long long wsum[SCAN_BLOCK / WAVE];
    const size_t base = (size_t) blockIdx.x * SCAN_TILE;
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        size_t i = base + (size_t) k * SCAN_BLOCK + threadIdx.x;   // strided: coalesced
        if (i < n) s += (unsigned long long) in[i];
    }
    s = waveReduceSumU64(s);
    if (laneId() == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < SCAN_BLOCK / WAVE; w++) t += wsum[w];
        partial[blockIdx.x] = t;
    }
}

// Exclusive scan of one tile per block; blockOff (nullable) supplies the scanned tile offsets.
// If writeTotal, the block that owns the end writes out[n] = grand total.
template <typename T>
__global__ __launch_bounds__(SCAN_BLOCK) void scanTileKernel(const T *in, uint64_t *out, size_t n,
                                                             const uint64_t *__restrict__ blockOff, int writeTotal) {
    __shared__ unsigned long long wsum[SCAN_BLOCK / WAVE];
    const size_t base = (size_t) blockIdx.x * SCAN_TILE + (size_t) threadIdx.x * SCAN_ITEMS;   // thread-contiguous
    unsigned long long v[SCAN_ITEMS];
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        size_t i = base + k;
        v[k] = (i < n) ? (unsigned long long) in[i] : 0ull;
        s += v[k];
    }
    unsigned long long incl = waveInclusiveScanU64(s);
    const int w = threadIdx.x >> 6;
    if (laneId() == 63) wsum[w] = incl;
    __syncthreads();
    unsigned long long woff = 0, tileTotal = 0;
#pragma unroll
    for (int j = 0; j < SCAN_BLOCK / WAVE; j++) { if (j < w) woff += wsum[j]; tileTotal += wsum[j]; }
    unsigned long long run = (blockOff ? blockOff[blockIdx.x] : 0ull) + woff + (incl - s);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        size_t i = base + k;
        if (i < n) out[i] = run;
        run += v[k];
    }
    if (writeTotal && threadIdx.x == 0) {
        const size_t lastBlock = (n == 0) ? 0 : (n - 1) / SCAN_TILE;
        if (blockIdx.x == lastBlock) out[n] = (blockOff ? blockOff[blockIdx.x] : 0ull) + tileTotal;
    }
}

size_t exclusiveScanTmpBytes(size_t n) {
    size_t bytes = 0;
    while (n > (size_t) SCAN_TILE) { size_t nb = (n + SCAN_TILE - 1) / SCAN_TILE; bytes += (nb + 1) * sizeof(uint64_t); n = nb; }
    return bytes + 64;
}

template <typename T>
static int scanImpl(hipStream_t stream, const T *d_in, uint64_t *d_out, size_t n, uint64_t *tmp) {
    if (n <= (size_t) SCAN_TILE) {
        hipLaunchKernelGGL(scanTileKernel<T>, dim3(1), dim3(SCAN_BLOCK), 0, stream, d_in, d_out, n, (const uint64_t *) nullptr, 1);
        return 0;
    }
    size_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scanReduceKernel<T>, dim3((unsigned) nb), dim3(SCAN_BLOCK), 0, stream, d_in, tmp, n);
    // NOTE: reduce reads strided within the tile while the downsweep reads thread-contiguous; both
    // cover exactly [tile*SCAN_TILE, (tile+1)*SCAN_TILE) so the per-tile sums agree.
    int rc = scanImpl<uint64_t>(stream, tmp, tmp, nb, tmp + nb + 1);
    if (rc) return rc;
    hipLaunchKernelGGL(scanTileKernel<T>, dim3((unsigned) nb), dim3(SCAN_BLOCK), 0, stream, d_in, d_out, n, (const uint64_t *) tmp, 1);
    return 0;
}

int exclusiveScanU32(hipStream_t stream, const uint32_t *d_in, uint64_t *d_out, size_t n, void *d_tmp, size_t tmpBytes) {
    if (tmpBytes < exclusiveScanTmpBytes(n)) return -1;
    return scanImpl<uint32_t>(stream, d_in, d_out, n, (uint64_t *) d_tmp);
}
int exclusiveScanU64(hipStream_t stream, const uint64_t *d_in, uint64_t *d_out, size_t n, void *d_tmp, size_t tmpBytes) {
    if (tmpBytes < exclusiveScanTmpBytes(n)) return -1;
    return scanImpl<uint64_t>(stream, d_in, d_out, n, (uint64_t *) d_tmp);
}

// ---- compactCsr: the flagged records of a CSR list, in input order ----
// A record is PIECES pieces of 16 bytes and a lane moves one piece, so both sides are coalesced whatever the record size.  (Every record
// array is the start of a poolMalloc block, and those are 256-byte aligned: core.hip, POOL_ALIGN — CandHit's own aligned(8) does not matter.)
template <int PIECES>
__global__ void compactRecsKernel(const uint4 *__restrict__ in, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ pos,
                                  uint4 *__restrict__ out, uint64_t n) {
    const uint64_t total = n * PIECES;
    for (uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t i = t / PIECES;
        if (keep[i]) out[pos[i] * PIECES + t % PIECES] = in[t];
    }
}
__global__ void compactOffsetsKernel(const uint64_t *__restrict__ inQoff, const uint64_t *__restrict__ pos, uint64_t *__restrict__ outQoff, uint64_t nQ) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i <= nQ; i += (uint64_t) gridDim.x * blockDim.x)
        outQoff[i] = pos[inQoff[i]];
}

int compactCsr(plasship_ctx *ctx, const char *what, const uint64_t *dInQoff, uint64_t nQ, const void *dRecs, size_t recBytes, const uint32_t *dKeep,
               uint64_t nRecs, uint64_t nKept, DevBuf &outQoff, DevBuf &outRecs) {
    // an early error return waits for the stream first: the caller's flag kernel may still be queued, and its flags are a local of the caller
    auto fail = [&](const char *msg, int rc) { (void) streamSync(ctx->stream); setError(std::string(what) + ": " + msg); return rc; };
    if (recBytes != 16 && recBytes != 64) return fail("internal error: records of 16 or 64 bytes only", PLASSHIP_ERR_ARG);
    DevBuf dPos, dTmp;
    const size_t tmpBytes = exclusiveScanTmpBytes(nRecs);
    if (dPos.alloc((nRecs + 1) * 8) != hipSuccess || dTmp.alloc(tmpBytes) != hipSuccess || outQoff.alloc((nQ + 1) * 8) != hipSuccess ||
        outRecs.alloc(std::max<uint64_t>(nKept, 1) * recBytes) != hipSuccess) return fail("out of device memory", PLASSHIP_ERR_DEVICE);
    if (exclusiveScanU32(ctx->stream, dKeep, dPos.as<uint64_t>(), nRecs, dTmp.p, tmpBytes)) return fail("scan failed", PLASSHIP_ERR_DEVICE);
    if (nRecs) {
        const uint64_t pieces = nRecs * (recBytes / 16);
        const dim3 grid((unsigned) std::min<uint64_t>((pieces + 255) / 256, (uint64_t) ctx->numCU * 64));
        if (recBytes == 16) hipLaunchKernelGGL(compactRecsKernel<1>, grid, dim3(256), 0, ctx->stream, (const uint4 *) dRecs, dKeep, dPos.as<uint64_t>(), outRecs.as<uint4>(), nRecs);
        else hipLaunchKernelGGL(compactRecsKernel<4>, grid, dim3(256), 0, ctx->stream, (const uint4 *) dRecs, dKeep, dPos.as<uint64_t>(), outRecs.as<uint4>(), nRecs);
    }
    hipLaunchKernelGGL(compactOffsetsKernel, dim3((unsigned) std::min<uint64_t>((nQ + 256) / 256, 65535)), dim3(256), 0, ctx->stream, dInQoff, dPos.as<uint64_t>(),
                       outQoff.as<uint64_t>(), nQ);
    // the one wait: the scan's total, after which dPos and dTmp may go (their kernels are through)
    uint64_t total = 0;
    PH_COPY_SYNC(ctx->stream, &total, dPos.as<uint64_t>() + nRecs, 8, hipMemcpyDeviceToHost);
    PH_CHECK(hipGetLastError());
    if (total != nKept) { setError(std::string(what) + ": internal error: the kept records do not add up to the list's count"); return PLASSHIP_ERR_DEVICE; }
    return PLASSHIP_OK;
}

// ---- RescoreList: the host side of a list-in, list-out rescoring call (common.hpp) ----
int RescoreList::prepare(size_t slotBytes_, bool wrapped, const double *evalThr, const plasship_clusters *subset) {
    const std::string w(what);
    slotBytes = slotBytes_;
    if (const int rc = refuseSharded(ctx, what)) return rc;
    if (c->nQueries != qdb->n) { setError(w + (tdb ? ": candidate list does not belong to the query DB" : ": candidate list does not belong to the DB")); return PLASSHIP_ERR_ARG; }
    if (tdb && qdb->dbtype != tdb->dbtype) { setError(w + ": query and target DB types differ"); return PLASSHIP_ERR_ARG; }
    nucl = qdb->dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES;
    if (wrapped && !nucl) { setError("Wrapped scoring is only supported for nucleotides."); return PLASSHIP_ERR_ARG; }      // rescorediagonal.cpp:70-76
    if (c->reverseCapable && !nucl) { setError(w + ": a candidate list with strands on a DB that is not nucleotides"); return PLASSHIP_ERR_ARG; }
    PH_ENTER(ctx);
    const uint64_t nHits = c->nHits;
    const size_t nQ = qdb->n;
    residues = (tdb ? tdb : qdb)->residues;
    if (subset) {
        if (const int rc = refuseForeign(what, subset, qdb)) return rc;
        std::vector<uint32_t> lens(nQ), repOf(nQ);
        PH_CHECK(streamSync(ctx->stream));
        if (nQ) { int rc = stagedCopyToHost(ctx, lens.data(), qdb->d_len.p, nQ * 4); if (!rc) rc = stagedCopyToHost(ctx, repOf.data(), subset->d_repOf.p, nQ * 4); if (rc) return rc; }
        residues = 0;
        for (size_t q = 0; q < nQ; q++) if (repOf[q] == q) residues += lens[q];
    }
    if (dKeep.alloc(std::max<uint64_t>(nHits, 1) * 4) != hipSuccess || dSlots.alloc(std::max<uint64_t>(nHits, 1) * slotBytes) != hipSuccess ||
        dStats.alloc(RL_NSTATS * 8) != hipSuccess || (evalThr && dMat.alloc(123 * 123) != hipSuccess)) {
        setError(w + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    PH_CHECK(hipMemsetAsync(dStats.p, 0, RL_NSTATS * 8, ctx->stream));
    args.hits = c->d_hits.as<CandHit>(); args.nHits = nHits; args.keep = dKeep.as<uint32_t>(); args.reverseCapable = c->reverseCapable;
    args.stats = dStats.as<unsigned long long>();
    if (evalThr) {
        const HostEvaluer ev(nucl, residues);
        if (const int rc = evalueGateTable(ctx, what, qdb, ev, *evalThr, dMinScore, hMinScore)) return rc;
        PH_CHECK(hipMemcpyAsync(dMat.p, asciiSubMat(nucl), 123 * 123, hipMemcpyHostToDevice, ctx->stream));
        args.minScore = dMinScore.as<uint32_t>(); args.minScoreLen = (uint32_t) hMinScore.size(); args.mat = dMat.as<signed char>();
        args.lambda = ev.g[0]; args.logK = ev.logK; args.ln2 = ev.ln2;
    }
    { int rc = ensureOffLen(ctx, qdb); if (!rc && tdb) rc = ensureOffLen(ctx, tdb); if (rc) return rc; }
    PH_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    return PLASSHIP_OK;
}

int RescoreList::collect(DevBuf &outQoff, DevBuf &outRecs, plasship_rescore_stats *stats) {
    PH_CHECK(hipEventRecord(ctx->ev[1], ctx->stream));
    unsigned long long hs[RL_NSTATS] = {};
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    if (hs[RL_BAD]) { setError(std::string(what) + (tdb ? ": the candidate list names sequences that are not in the DBs" : ": the candidate list names sequences that are not in the DB")); return PLASSHIP_ERR_ARG; }
    nKept = hs[RL_KEPT]; nNonSelf = hs[RL_VISIBLE];
    if (const int rc = compactCsr(ctx, what, c->d_qoff.as<uint64_t>(), qdb->n, dSlots.p, slotBytes, dKeep.as<uint32_t>(), args.nHits, nKept, outQoff, outRecs)) return rc;
    if (stats) {
        stats->n_scored = args.nHits; stats->n_accepted = nKept; stats->overlap_residues = hs[RL_RESIDUES];
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); stats->ms_kernel = ms;
    }
    return PLASSHIP_OK;
}

}  // namespace plasship
