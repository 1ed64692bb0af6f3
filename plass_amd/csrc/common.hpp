// plasship internal declarations (product code; never includes anything from oracle/).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <map>
#include <vector>
#include "../../include/plasship.h"

namespace plasship {

void setError(const std::string &msg);
// every wait of the host for the stream goes through here and is counted (plasship_host_syncs(): bench.py reports waits per iteration)
hipError_t streamSync(hipStream_t st);
}
struct plasship_seqdb; struct plasship_ctx;
namespace plasship {
int ensureOffLen(plasship_ctx *ctx, const plasship_seqdb *db);     // core.hip: builds plasship_seqdb::d_offLen once (stream-ordered)
std::string hipErrStr(hipError_t e, const char *what, const char *file, int line);

#define PH_CHECK(call)                                                                   \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            plasship::setError(plasship::hipErrStr(e_, #call, __FILE__, __LINE__));     \
            return PLASSHIP_ERR_DEVICE;                                                  \
        }                                                                                \
    } while (0)
// The context stream is non-blocking: a plain hipMemcpy runs on the null stream and is NOT ordered with work queued on
// it.  Every blocking copy in the library goes through this: queued on the context stream, then waited for.
#define PH_COPY_SYNC(st, dst, src, bytes, kind)                                          \
    do {                                                                                 \
        PH_CHECK(hipMemcpyAsync((dst), (src), (bytes), (kind), (st)));                   \
        PH_CHECK(plasship::streamSync(st));                                              \
    } while (0)

// the switches of the build: PLASSHIP_TUNE_<name> in the environment, or dflt when it is unset or <= 0.  What is left of the rounds' A/B
// dials is what a test or tool sets, or what turns an optimisation off to bisect a wrong result or cap memory; the names are listed in
// core.hip (TUNE_NAMES), and any other PLASSHIP_TUNE_<x> is reported when the first context is created.  (The grids of the persistent
// kernels are constants now; they were swept with these dials: the best grid is the number of workgroups a CU holds at once, or a small
// multiple — one more leaves a tail round: extractShortKernel: 18 -> 0.69 ms, 20 -> 0.81 ms.)
int tuneInt(const char *name, int dflt);
// PLASSHIP_TRACE=1: wait for the stream at every marked stage boundary and say so on stderr (localises a faulting kernel)
bool traceOn();
#define PH_TRACE(st, what)                                                                \
    do {                                                                                 \
        if (plasship::traceOn()) {                                                       \
            hipError_t e_ = plasship::streamSync(st);                                    \
            fprintf(stderr, "[plasship] %s: %s\n", (what), hipGetErrorString(e_));       \
        }                                                                                \
    } while (0)

// Caching device allocator: hipMalloc/hipFree synchronise the device and cost 0.1–1 ms each, which would
// dominate an assembly iteration on a 1 M-read set.  Freed blocks are kept (size classes with <= 12.5 % slack)
// and handed out again; everything is returned to HIP when the last context is destroyed or on out-of-memory.
// longLived: a buffer that outlives the module call that makes it (sequence DBs and their heaps, the selected-window cache).  It is
// placed at the TOP of the highest free range that holds it instead of at the front of the best-fitting one, so that the long-lived
// buffers collect at one end of the arena and the 60 GB record arrays of kmermatcher keep finding contiguous room (round 4: with
// heaps and cache lines scattered over the arena the 50 M-read chain ran out of memory with 80 GB free).
hipError_t poolMalloc(void **p, size_t n, bool longLived = false);
// every C-ABI entry that allocates calls this first (PH_ENTER): the stream the calling thread's allocations belong to
void poolEnter(hipStream_t stream);
// sharded run (round 6): which rank the calling thread's context is, so that a wait for the stream that never ends — a collective a peer
// never joined, a link that is down: what the FIRST run on real xGMI links can meet — becomes an error with the rank and the last
// collective in it instead of a hang (core.hip: streamSync polls with a deadline when a communicator of more than one rank is installed;
// PLASSHIP_COMM_TIMEOUT_S, default 300, 0 = wait for ever).  watchCollective names what was enqueued last.
void watchEnter(const plasship_ctx *ctx);
void watchCollective(const char *what);
#define PH_ENTER(ctx)                                                                    \
    do {                                                                                 \
        PH_CHECK(hipSetDevice((ctx)->device));                                           \
        plasship::poolEnter((ctx)->stream);                                              \
        plasship::watchEnter(ctx);                                                       \
    } while (0)
void poolFree(void *p);
void poolTrim();

// RAII device buffer (untyped bytes)
struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t n, bool longLived = false) { release(); bytes = n; if (n == 0) { p = nullptr; return hipSuccess; } return poolMalloc(&p, n, longLived); }
    hipError_t allocLong(size_t n) { return alloc(n, true); }
    void release() { if (p) { poolFree(p); p = nullptr; } bytes = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- device-side views (POD, passed to kernels by value) --------------------------------------
struct SeqView {
    const char *data;          // entries "SEQ\n\0"
    const uint64_t *off;       // [n] byte offset of entry i (id = rank in key order)
    const uint32_t *len;       // [n] sequence length (entry length - 2)
    const uint64_t *offLen;    // [n] off << 24 | len in one word, or nullptr (ensureOffLen): ONE line instead of two for a random entry
    uint32_t n;
    int nucl;
};

#ifdef __HIPCC__
// offset / length of a RANDOM entry from the packed word (requires ensureOffLen on the DB)
__device__ __forceinline__ uint64_t seqOff(const SeqView &s, uint32_t id) { return s.offLen[id] >> 24; }
__device__ __forceinline__ uint32_t seqLen(const SeqView &s, uint32_t id) { return (uint32_t) s.offLen[id] & 0xFFFFFFu; }
#endif

// one candidate pair (query id implied by CSR)
struct __attribute__((aligned(8))) CandHit { uint32_t target; int32_t prefScore; uint32_t diag16; uint32_t query; };

// one scored/accepted alignment (device + host layout)
struct AlnRec {
    uint32_t query, target;    // ids (ranks)
    int32_t bitScore, rawScore;
    float seqId;               // exact float (or parsed text value if fromText)
    int32_t qStart, qEnd, qLen, dbStart, dbEnd, dbLen, alnLen;
    int32_t reversed;
    int32_t accepted;
    int32_t fromText;
    int32_t btKind;            // backtrace of the record: 0 unknown / none, 1 one run of alnLen 'M' (ungapped), 2 anything else,
                               // ALN_SELF_PENDING: an identity pair not scored yet (plasship_alns::selfPending)
};
constexpr int32_t ALN_SELF_PENDING = 3;

// the selection parameters of one plasship_kmermatch call (host only): what two calls must share for the later one to reuse what the
// earlier one selected.  alph: the alphabet the k-mer index is built over (5 for nucleotides); lng: the 24-byte record layout
struct KmSelect {
    int k = 0, alph = 0, kps = 0; float scale = 0; int ignoreMulti = 0, hashShift = 0; bool lng = false;
    bool operator==(const KmSelect &o) const {
        return k == o.k && alph == o.alph && kps == o.kps && scale == o.scale && ignoreMulti == o.ignoreMulti && hashShift == o.hashShift && lng == o.lng;
    }
};

}  // namespace plasship

struct plasship_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[16] = {};
    int numCU = 0;
    // nuclassembleresults: comparator decisions that lie on a threshold, resolved with the host libm (assemble.hip);
    // kept for the lifetime of the context (the same few (alpha, beta) tuples recur in every iteration)
    std::vector<uint32_t> ambKeys;      // 4 words per entry
    std::vector<uint8_t> ambVals;
    plasship::DevBuf d_ambKeys, d_ambVals;
    plasship::DevBuf d_cmpCache;        // memo of the nucleotide comparator's posterior classes (assemble.hip, nuclLess)
    uint32_t ambSlots = 0;              // power of two, 0 = no table yet
    // host boundary: two pinned staging buffers (allocated on first use) every bulk host<->device copy goes through — a chunk is
    // packed / consumed on the host threads while the previous one is on the PCIe link (stagedUpload / stagedDownload, core.hip)
    char *stage[2] = {nullptr, nullptr};
    hipEvent_t stageEv[2] = {nullptr, nullptr};
    size_t stageBytes = 0;
    void *pinnedTable = nullptr;        // 1 MB of pinned host memory for small tables a kernel chain reads (ctxPinnedTable, core.hip)
    // one read set sharded over several GPUs (plasship_ctx_set_comm); world == 1 and hasComm == false: single GPU
    bool hasComm = false;
    plasship_comm comm = {};
    int debugFailCollective = -1;       // plasship_ctx_debug_fail_collective: countdown to an injected rank-local failure
    // kmermatcher's selected-window cache (kmermatch.hip section 2c): per sequence one 128-byte line {identity-record hash, the positions
    // of the <= 60 selected k-mers} of the LAST plasship_kmermatch call on this context; the next call re-uses the line of every
    // sequence its DB inherited unchanged from that call's DB when the selection parameters (hash seed included) are the same
    struct KmCache {
        plasship::DevBuf lines; uint64_t n = 0, gen = 0; bool valid = false, seenEligible = false;      // seenEligible: an earlier call on this context could have used lines (they are allocated from the second such call on, or for a derived DB)
        plasship::KmSelect sel;         // of the call that wrote the lines
    } kmCache;
    // kmermatcher's position cache of nucleotide runs (kmermatch_extract.hpp section 2d): per record slot of the LAST nucleotide
    // plasship_kmermatch call on this context the window position it selected (the identity slot: the count), that call's slot offsets
    // and identity hashes.  `gen` (that call's DB) is the ANCHOR: every DB buildOutputDB derives from it, directly or through other derived
    // DBs, carries per entry the id it had in the anchor (plasship_seqdb::d_origin) — entries may be dropped on the way.
    struct KmPosCache {
        plasship::DevBuf pos, slotOff, idHash; uint64_t n = 0, gen = 0; bool valid = false, seen = false;
        plasship::KmSelect sel;         // of the call that wrote the positions
    } kmPosCache;
    uint64_t kmermatchCalls = 0;       // plasship_kmermatch calls this context has seen (a second call suggests a chain: the caches are written from then on)
    // cyclecheck.hip: generation of the last "rest" DB plasship_cyclecheck made on this context (every entry of it is known not to be
    // circular at that --max-seq-len); a later call on a DB that descends from it checks only the entries rewritten since
    uint64_t cycKnownGen = 0, cycKnownMaxLen = 0;
    // orfs.hip: the device tables (complement, gap, base codes, residue LUT) of every genetic code but the standard one that this context
    // has extracted or translated with, by --translation-table id; uploaded on first use
    std::map<int, plasship::DevBuf> gencodeTables;
};

namespace plasship {
uint64_t newDbGeneration();
// An append-only byte heap shared by a chain of sequence DBs (outdb.hip, buildOutputDB): an assembly iteration changes 10-20 % of
// the sequences, so the DB it makes keeps the bytes of the unchanged entries where they are — its index points into the heap of the
// DB it derives from — and only the extended entries are appended behind `used`.  Nothing is ever overwritten, so every DB of the
// chain stays valid for as long as its handle lives; the buffer goes when the last of them does.
struct SeqHeap { DevBuf buf; std::atomic<uint64_t> used{0}; };
}      // core.hip: a process-wide counter; every sequence DB handle gets its own number
struct plasship_seqdb {
    int dbtype = 0;
    // Lineage (kmermatch.hip, the selected-window cache): `gen` names this handle; a DB that buildOutputDB derived from another one
    // WITHOUT dropping entries (same ids, same keys) names it in `parentGen` and marks in d_changed (one byte per id) the entries whose
    // bytes differ from the parent's.  0 = no such parent (read from disk, generated, concatenated, entries dropped).
    // `ancestorGen` is the weaker statement that survives dropped entries (nuclassembleresults removes the consumed targets): every
    // entry with d_changed == 0 is byte for byte an entry of the DB with that generation, under whatever id (cyclecheck.hip).
    uint64_t gen = plasship::newDbGeneration(), parentGen = 0, ancestorGen = 0;
    plasship::DevBuf d_changed;
    // `originGen` != 0: d_origin[i] = the id entry i had in the DB of that generation (the anchor of kmermatcher's position cache,
    // plasship_ctx::kmPosCache), 0xFFFFFFFF if its bytes are not an entry of that DB; survives dropped entries and chains of derivations
    uint64_t originGen = 0;
    plasship::DevBuf d_origin;
    size_t n = 0;
    uint64_t dataBytes = 0, residues = 0;
    uint32_t maxEntryLen = 0;
    plasship::DevBuf d_data, d_off, d_len, d_key;
    // heap != nullptr: the entries' bytes are in heap->buf (d_data is empty) at d_off[i], NOT necessarily back to back or in key order;
    // `contiguous` says whether they are (a freshly compacted heap is; then, like d_data, the bytes [0, dataBytes) are the data file)
    std::shared_ptr<plasship::SeqHeap> heap;
    bool contiguous = true;
    uint64_t buildAppendedBytes = 0, buildCopiedBytes = 0;  // how buildOutputDB made this DB: bytes appended to the shared heap / bytes of a full copy
    // a subset (plasship_select_contigs) of a DB without a heap indexes that DB's own buffer, which must outlive it
    const char *borrowedData = nullptr;
    const char *dataPtr() const { return heap ? heap->buf.as<char>() : borrowedData ? borrowedData : d_data.as<char>(); }
    // rank of every entry in DATA FILE order (empty: the file lay in key order, rank == id).  Only DBs read from files written by
    // several threads have one; concatdbs renumbers its second DB by it (DBConcat.cpp:46-47,113-118 opens it LINEAR_ACCCESS).
    plasship::DevBuf d_fileRank;
    // offset and length of every entry packed into one word (plasship::ensureOffLen): the kernels that look up RANDOM entries
    // (the targets of candidate pairs and alignments) fetch one line per entry instead of one of d_off and one of d_len
    mutable plasship::DevBuf d_offLen;
    // (built lazily on the stream of the first context that needs it; a second context on the same handle — the chain driver's writer
    //  thread, ranks sharing a DB — takes the lock and waits for that kernel on its own stream: ensureOffLen, core.hip)
    mutable std::mutex offLenMu; mutable hipEvent_t offLenEv = nullptr; mutable hipStream_t offLenStream = nullptr;
    ~plasship_seqdb() { if (offLenEv) (void) hipEventDestroy(offLenEv); }
    // host mirror of the index (lazily filled for device-produced DBs)
    bool hostIndexValid = false;
    std::vector<uint32_t> h_key, h_elen;
    std::vector<uint64_t> h_off;
    plasship::SeqView view() const {
        plasship::SeqView v; v.data = dataPtr(); v.off = d_off.as<uint64_t>(); v.len = d_len.as<uint32_t>(); v.offLen = d_offLen.as<uint64_t>();
        v.n = (uint32_t) n; v.nucl = (dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES); return v;
    }
};

struct plasship_cands {
    bool reverseCapable = false;   // DBTYPE_PREFILTER_REV_RES
    size_t nQueries = 0;           // == query DB size; every query has an entry
    uint64_t nHits = 0;            // including the explicit self hits
    uint64_t nNonSelf = 0;
    plasship::DevBuf d_qoff;       // uint64 [nQueries+1]
    plasship::DevBuf d_hits;       // CandHit [nHits], sorted by (query, target order of the reference)
    // plasship_cands_filter only: h_present[q] == 0: query q has no entry at all (createsubdb removed it), so plasship_cands_write leaves it
    // out instead of writing an empty entry.  Empty (every other list): every query has an entry.
    std::vector<uint8_t> h_present;
};

// every sequence of a DB with its representative, as the cluster DB lists them: what the clustering family's handles share (clust_shared.hpp)
namespace plasship {
struct PairList {
    size_t n = 0;                  // == DB size
    uint64_t nClusters = 0;
    uint64_t dbGen = 0;            // plasship_seqdb::gen of the DB it was made on
    DevBuf d_pairs;                // uint64 [n]: representative id << 32 | member id (ids are ranks in key order: the keys' order)
};
}
// a clustering (clust.hip, clust_cc.hip, plasship_clusters_read): the pairs ascending
struct plasship_clusters : plasship::PairList {
    plasship::DevBuf d_repOf;      // uint32 [n]: the representative's id of every id
};
// what plasship_clusters_merge makes (include/plasship_ext/linclust.h): the pairs in the order of the merged DB
struct plasship_merged : plasship::PairList {};

struct plasship_alns {
    size_t nQueries = 0;
    uint64_t nLines = 0;           // ACCEPTED alignments (what plasship_alns_count reports, what a DB file holds)
    // Round 5: a list made by plasship_rescore is SPARSE — one record slot per candidate pair, in the candidate list's own CSR, a rejected
    // pair's record carrying accepted == 0 — because 95 % of the pairs of an assembly iteration are accepted: compacting the list moved
    // 38 GB per iteration (8 ms at 50 M reads) to close 5 % of holes.  Every kernel that walks a query's records skips the holes (the
    // extension kernels' queue fill, arenaSumKernel, findStartVoteKernel, aln2nuclKernel); the host paths (download, DB files) take a
    // dense copy first (denseAlnsCopy, rescore.hip).  Lists read from DB files or made dense are not sparse: nSlots == nLines.
    uint64_t nSlots = 0;           // records in d_recs (holes included)
    bool sparse = false;
    // Round 5, LAZY SELF HITS: every query's alignment with itself (a third of the pairs, and in the late iterations of an assembly — contigs of
    // thousands of residues against themselves — most of the columns rescorediagonal scores: the stage grew 20 -> 60 ms over the twelve
    // iterations at 50 M reads while the candidate pairs fell) is accepted whatever it scores, and assembleresults pops and discards it
    // (assembleresult.cpp:203-209, isNotIdentity), findassemblystart skips it.  plasship_rescore therefore leaves the identity pairs as STUBS
    // (accepted = 1, btKind = ALN_SELF_PENDING, the candidate's score / diagonal stashed in rawScore / qStart) and the first consumer that
    // READS a self record — DB files, downloads, proteinaln2nucl, the nucleotide and guided extension (whose comparator ranks the self hit
    // with the others) — has them scored then, by the same kernels (finishSelfAlns, rescore.hip): every record any reader sees is the
    // record rounds 1-4 made.  selfPending is the list's state, not its value: mutable, set back by finishSelfAlns.
    mutable bool selfPending = false;
    plasship_rescore_params rsPar = {};      // what finishSelfAlns scores with
    bool rsSameDB = false; int rsReverseCapable = 0;
    bool nucl = false;
    bool addBacktrace = false;
    uint64_t dbResidues = 0;       // of the target DB (E-value area)
    int gappedOpen = 0, gappedExtend = 0;   // != 0: E-values of the gapped nucleotide evaluer (list made by plasship_aln2nucl)
    plasship::DevBuf d_qoff;       // uint64 [nQueries+1]
    plasship::DevBuf d_recs;       // AlnRec [nSlots]
    // DBs the list refers to (ids -> keys for text output); they must outlive this object
    const plasship_seqdb *qdb = nullptr, *tdb = nullptr;
};

namespace plasship {
// ---- what the single-GPU modules refuse, in the words every one of them uses; what: the public call the text names ----
inline int refuseSharded(const plasship_ctx *ctx, const char *what) {
    if (ctx->hasComm && ctx->comm.world > 1) { setError(std::string(what) + ": not part of a sharded run (a communicator of more than one rank is set)"); return PLASSHIP_ERR_UNSUPPORTED; }
    return PLASSHIP_OK;
}
inline int refuseForeign(const char *what, const PairList *list, const plasship_seqdb *db) {
    if (list->n != db->n || list->dbGen != db->gen) { setError(std::string(what) + ": the clustering does not belong to this DB"); return PLASSHIP_ERR_ARG; }
    return PLASSHIP_OK;
}
inline int refuseWideIds(const char *what, const plasship_seqdb *db) {
    if (db->n >= 0xFFFFFFFFull) { setError(std::string(what) + ": ids are 32-bit"); return PLASSHIP_ERR_UNSUPPORTED; }
    return PLASSHIP_OK;
}
// the grid of a flat grid-stride kernel of 256 threads over n items: enough workgroups for n, at most 32 per CU, at least one
inline unsigned flatGrid(uint64_t n, int numCU) { return (unsigned) std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t) numCU * 32)); }

// ---- sharded operation (comm.hip): thin wrappers over the caller's collectives; all of them synchronise the stream first ----
inline const plasship_comm *commOf(const plasship_ctx *ctx) { return ctx->hasComm ? &ctx->comm : nullptr; }
// first id owned by rank r of `world` when n ids are split into contiguous ranges: ceil(r*n/world)
inline uint64_t ownedBegin(uint64_t n, int r, int world) { return ((uint64_t) r * n + (uint64_t) world - 1) / (uint64_t) world; }
int commAllgatherHost(plasship_ctx *ctx, const void *send, void *recv, uint64_t bytesPerRank);
int commAllReduceSumU64(plasship_ctx *ctx, uint64_t *v, size_t n);       // in place
int commAllReduceMaxU64(plasship_ctx *ctx, uint64_t *v, size_t n);
int commAllReduceMinU64(plasship_ctx *ctx, uint64_t *v, size_t n);
int commAgreeOk(plasship_ctx *ctx, bool ok, const char *what);          // collective: error on every rank unless `ok` on every rank
// Failure protocol of a sharded call (comm.hip): every collective starts with an 8-byte status round; a rank that fails on its own
// between two collectives returns to its C-ABI entry, whose commFinish() sends its error code as the status of ONE more round — the
// round the other ranks make before their next collective, or their own commFinish() — and every rank leaves the call with an error
// (PLASSHIP_ERR_PEER on the ranks that did not fail themselves).  Nobody is left waiting inside a collective.
int commFinish(plasship_ctx *ctx, int rc);                              // last statement of every C-ABI entry that can run sharded
// all-to-all(v) of fixed-size records laid out by destination; allocates `recv` (capacity (total + slackRecords) records)
// *allTotal (optional): records sent by all ranks together
int commAlltoallvRecords(plasship_ctx *ctx, const void *dSend, const uint64_t *sendCount, size_t recordBytes, DevBuf &recv,
                         uint64_t *recvTotal, uint64_t slackRecords, uint64_t *allTotal = nullptr);
// all-gather(v) of bytes; allocates `recv`; recvBytes[world] / recvOff[world+1] filled
int commAllgathervBytes(plasship_ctx *ctx, const void *dSend, uint64_t sendBytes, DevBuf &recv, std::vector<uint64_t> &recvBytes);
// the same when every rank already knows everybody's size (recvBytes[world] given)
int commAllgathervBytesKnown(plasship_ctx *ctx, const void *dSend, uint64_t sendBytes, DevBuf &recv, const std::vector<uint64_t> &recvBytes);
// ---- the output-DB writer (outdb.hip) ----
// where buildOutputDB puts the entries of the DB it makes
enum class OutPlacement {
    // the DB shares `db`'s heap (SeqHeap) when it has one with room: only the rewritten entries move.  Otherwise it opens a new heap with
    // slack for the iterations to come (PLASSHIP_TUNE_DBHEAP=2: no heaps, an exact buffer of its own).  Lineage and origin are recorded.
    Chain,
    // back to back in key order in an exact buffer — the layout of the DB file — with lineage and origin.  For the DBs of the protein-guided
    // path: the reference's proteinaln2nucl and guidedassembleresults read PAST the end of an entry when a protein twin and its ORF / 3
    // differ in length, i.e. into the entry that FOLLOWS in the data file; behind an entry appended to a shared heap
    // lies whatever was appended next.  tests/test_gpu_deep.py::test_four_guided_iterations (round 5) found the difference in the third
    // guided iteration, the first one whose input DB had appended entries: 3 bytes of one alignment DB in 382 MB.  Also for a DB nobody
    // will ever append behind (cyclecheck's cycle DB): no slack.
    Exact,
    // a packed copy in an exact buffer, no lineage, no origin (packedCopyOf)
    Packed
};
// what differs from `db`: entries with flag 0x20 come from `arena + newStart[id]` (newLen[id] residues), the others are carried over
// from `db` (dropped when !keepTarget and flag 0x80 is set)
struct OutEdits { const uint32_t *flags = nullptr; const uint32_t *newLen = nullptr; const uint64_t *newStart = nullptr; const char *arena = nullptr; int keepTarget = 0; };
struct OutOptions {
    OutPlacement placement = OutPlacement::Chain;
    hipEvent_t doneEvent = nullptr;       // recorded behind the writer's last kernel
    const void *dExtra = nullptr; void *hExtra = nullptr; size_t extraBytes = 0;       // the caller's counters ride along with the writer's last copy to the host
};
// builds an output sequence DB in key order (outdb.hip) from `db` and the edits
int buildOutputDB(plasship_ctx *ctx, const plasship_seqdb *db, const OutEdits &edits, void *dTmp, size_t tmpBytes, plasship_seqdb **out, const OutOptions &opt = {});
// a copy of `db` with its entries back to back in key order in a buffer of its own (outdb.hip); callers that stream or copy the
// data of a DB as one block (DB files, downloads, concatdbs) take it when !db->contiguous
int packedCopyOf(plasship_ctx *ctx, const plasship_seqdb *db, std::unique_ptr<plasship_seqdb> &out);
// ---- host boundary (core.hip): bulk copies through the context's pinned double buffer, on the context stream ----
// H2D of `total` bytes the caller produces chunk by chunk: produce(dst, byteOffset, bytes) fills a pinned chunk (consecutive chunks,
// in order; it may use the host threads) while the previous chunk is in flight.  Returns after the last copy has completed.
// chunk != 0: chunks of that many bytes (at most a staging buffer); enqueued(end) runs after the copy of the bytes [.., end) has been put on
// the stream — kernels it launches there work on that chunk while the next one is produced and copied (createdb.hip); non-zero aborts.
int stagedUpload(plasship_ctx *ctx, void *dDst, uint64_t total, const std::function<void(char *, uint64_t, uint64_t)> &produce,
                 uint64_t chunk = 0, const std::function<int(uint64_t)> *enqueued = nullptr);
// D2H: consume(src, byteOffset, bytes) sees consecutive chunks in order (false aborts with PLASSHIP_ERR_IO); the next chunk is
// already being copied while it runs
int stagedDownload(plasship_ctx *ctx, const void *dSrc, uint64_t total, const std::function<bool(const char *, uint64_t, uint64_t)> &consume);
// 1 MB of pinned host memory owned by the context (nullptr if `bytes` does not fit or it cannot be allocated): a table copied from
// it with hipMemcpyAsync needs no wait before the host moves on.  One user per module call; the next call's use comes after that
// call's own waits, by which time the copy has long completed.
void *ctxPinnedTable(plasship_ctx *ctx, size_t bytes);
// plain arrays: host -> device / device -> host through the staging buffers (memcpy on the host threads)
int stagedCopyToDevice(plasship_ctx *ctx, void *dDst, const void *hSrc, uint64_t bytes);
int stagedCopyToHost(plasship_ctx *ctx, void *hDst, const void *dSrc, uint64_t bytes);
// sets *differ when two key arrays (device, n entries) are not identical
int deviceKeysDiffer(plasship_ctx *ctx, const uint32_t *a, const uint32_t *b, size_t n, bool *differ);
// orfs.hip: extractorfs / translatenucs with any genetic code and the codes' strings; libplasship_gencode.so exports them (include/plasship_ext/gencode.h)
int gencodeInfo(int table, char residues[65], char starts[65]);
int extractOrfsGencode(plasship_ctx *ctx, const plasship_seqdb *reads, const plasship_orf_params *par, plasship_seqdb **out_orfs, plasship_orfhdr **out_hdr, plasship_orf_stats *stats);
int translateNucsGencode(plasship_ctx *ctx, const plasship_seqdb *orfs, const plasship_orfhdr *hdr, const plasship_translate_params *par, plasship_seqdb **out_aa, plasship_orf_stats *stats);
// The flagged records of a CSR list (scan.hip): outRecs = the records with dKeep[i] != 0, in input order; outQoff[q] = the number of kept
// records before dInQoff[q], q in [0, nQ].  recBytes is 16 (CandHit) or 64 (AlnRec).  nKept is what the caller counted: it sizes outRecs
// (max(nKept, 1) records) and is checked against the scan's total.  Waits for the stream exactly once, at its end (on an
// error too); dKeep may go after it.  what: the public call or list the error texts name.
int compactCsr(plasship_ctx *ctx, const char *what, const uint64_t *dInQoff, uint64_t nQ, const void *dRecs, size_t recBytes, const uint32_t *dKeep,
               uint64_t nRecs, uint64_t nKept, DevBuf &outQoff, DevBuf &outRecs);
// The E-value gate of rescorediagonal as a table (rescore.hip): hMinScore[l] = the smallest raw score that passes -e evalThr for a query of
// length l, for every length qdb holds (0xFFFFFFFF elsewhere), uploaded to dMinScore.  Exact, because E(score) is monotone (host_util.cpp).
// Waits for the stream once; the upload is only queued: hMinScore must live until the caller's next wait.
struct HostEvaluer;
int evalueGateTable(plasship_ctx *ctx, const char *what, const plasship_seqdb *qdb, const HostEvaluer &ev, double evalThr, DevBuf &dMinScore,
                    std::vector<uint32_t> &hMinScore);
// ---- list-in, list-out rescoring (scan.hip): what plasship_rescore_hamming, plasship_rescore_local[_subset] and
// plasship_rescore_subst[_subset] do around their kernels ----
enum RescoreStat { RL_KEPT, RL_RESIDUES, RL_VISIBLE, RL_BAD, RL_NSTATS };      // pairs kept, residues compared or scored, kept lines that are not an implicit self line, ids out of range
// what every one of these kernels is handed
struct RescoreListArgs {
    const CandHit *hits;
    uint64_t nHits;
    uint32_t *keep;              // [nHits] 1: the pair's line or record is written (slot h belongs to pair h)
    const uint32_t *minScore;    // [minScoreLen] evalueGateTable
    uint32_t minScoreLen;
    const signed char *mat;      // 123 x 123 in global memory, staged to LDS
    int reverseCapable;
    double lambda, logK, ln2;
    unsigned long long *stats;   // [RL_NSTATS]
};
struct RescoreList {
    plasship_ctx *ctx; const char *what;                     // what: the public call the error texts name
    const plasship_seqdb *qdb, *tdb;                         // tdb == nullptr: one DB is query and target
    const plasship_cands *c;
    // after prepare()
    bool nucl = false; size_t slotBytes = 0;
    uint64_t residues = 0;                                   // the E-value's database size
    DevBuf dKeep, dSlots, dStats, dMinScore, dMat;
    std::vector<uint32_t> hMinScore;
    RescoreListArgs args = {};
    // after collect()
    uint64_t nKept = 0, nNonSelf = 0;
    // The shared argument checks, the buffers (slots of slotBytes per pair), the tables and the first event; the kernel is launched after it.
    // evalThr == nullptr: no E-value table and no matrix (mode 0).  subset: the E-value's database size is the residue count of its
    // representatives.
    int prepare(size_t slotBytes, bool wrapped, const double *evalThr, const plasship_clusters *subset);
    // The second event, the counters, the kept slots in input order with the CSR over them (compactCsr), and `stats` (nullable)
    int collect(DevBuf &outQoff, DevBuf &outRecs, plasship_rescore_stats *stats);
};
// dense (hole-free) copy of an alignment list's CSR and records on the device (rescore.hip); for a list that is not sparse the buffers
// stay empty and *qoff / *recs point at the list's own arrays
int denseAlnsCopy(plasship_ctx *ctx, const plasship_alns *a, DevBuf &qoffBuf, DevBuf &recsBuf, const uint64_t **qoff, const AlnRec **recs);
// scores the identity pairs plasship_rescore left as stubs (plasship_alns::selfPending); no-op for a list that has none
// (dQueryList: only the stubs of these nQueryList queries — ids on the device)
int finishSelfAlns(plasship_ctx *ctx, const plasship_alns *a, const uint32_t *dQueryList = nullptr, uint32_t nQueryList = 0);
}
