// plass-hip: the reference's module command lines over the plasship C-ABI.
//
// The reference workflow scripts run `"$MMSEQS" <module> <dbs…> <flags…>` (data/assemble.sh:43-145); pointing $MMSEQS at this
// binary for the hot modules makes them run on the MI355X while every database on disk keeps the DBReader/DBWriter format.
// Module names, positional arguments and flag names are the reference's (mm/commons/Parameters.cpp:423-439,640-655,763-767,
// 872-892,970-974; src/commons/LocalParameters.h:96-117,171-176).  Parsing follows Parameters::parseParameters
// (Parameters.cpp:1560-1700): a flag the module does not own is an error, a bool flag without a value toggles its default, and
// defaults are the MODULE's defaults (Parameters::setDefaults, setLinearFilterDefault), not the assemble workflow's — a call
// that does not come from createParameterString therefore means the same thing here and there.  Flags that cannot influence
// the result (--threads, -v, --db-load-mode, --compressed 0 …) are accepted and ignored; values this build cannot honour
// (another substitution matrix, spaced k-mers, masking, automatic k …) fail loudly like Debug(Debug::ERROR) + EXIT(EXIT_FAILURE).
#include "../../include/plasship.h"
#include "../../include/plasship_ext/clust.h"
#include "../../include/plasship_ext/linclust.h"
#include "../../include/plasship_ext/subst.h"
#include "../../include/plasship_ext/cc.h"
#include "../../include/plasship_ext/gencode.h"
#include <chrono>
#include <unistd.h>
#include <cstdarg>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <sys/stat.h>
#include <vector>

static bool multiParam(const std::string &v, const char *which, std::string &out) {
    if (v.find(':') == std::string::npos) { out = v; return true; }
    size_t p = 0;
    while (p < v.size()) {
        size_t c = v.find(',', p); if (c == std::string::npos) c = v.size();
        std::string part = v.substr(p, c - p);
        size_t col = part.find(':');
        if (col != std::string::npos && part.substr(0, col) == which) { out = part.substr(col + 1); return true; }
        p = c + 1;
    }
    return false;
}
static std::string baseName(const std::string &p) { const size_t s = p.find_last_of('/'); return s == std::string::npos ? p : p.substr(s + 1); }
static int frameMask(const std::string &v, bool &ok) {                   // Orf::getFrames: "1,2,3"
    int m = 0; size_t p = 0; ok = true;
    while (p <= v.size()) {
        size_t c = v.find(',', p); if (c == std::string::npos) c = v.size();
        const std::string t = v.substr(p, c - p);
        if (!t.empty()) { const int f = atoi(t.c_str()); if (f < 1 || f > 3) ok = false; else m |= 1 << (f - 1); }
        p = c + 1;
    }
    return m;
}

struct Flags {
    // Parameters::setDefaults (Parameters.cpp:2093-2338); kmermatcher additionally setLinearFilterDefault (kmermatcher.cpp:566-573)
    int k = 0, alph = 21, kps = 21, hashShift = 67, onlyExt = 0, ignoreMulti = 0, covMode = 0;
    float scaleAA = 0.0f, scaleNucl = 0.2f, covThr = 0.0f, seqIdThr = 0.0f;
    int rescoreMode = 0, minAlnLen = 0, seqIdMode = 0, addBt = 0, addSelf = 0, keepTarget = 1, wrapped = 0, filterHits = 0, sortResults = 0;
    double evalThr = 1e-3;
    unsigned long long maxSeqLen = 65535;
    int gapOpenNucl = 5, gapExtendNucl = 2;
    int chopCycle = 1;                   // LocalParameters.h:202
    int orfMin = 30, orfMax = 32734, orfGaps = INT_MAX, contigStart = 2, contigEnd = 2, orfStart = 1, fwdFrames = 7, revFrames = 7;
    int translationTable = 1, translate = 0, allStarts = 0, addOrfStop = 0, preserveKeys = 0, takeLarger = 0;
    int numIterations = 0, fromReads = 0, resume = 0; std::string writeIntermediate; float seqIdThrNucl = 0.99f;
    // the workflows' tail (--fasta-out): Assembler.cpp / Nuclassembler.cpp defaults (--filter-proteins 1, --min-contig-len 1000,
    // --contig-output-mode 1)
    std::string fastaOut; int filterProteins = 1, minContigLen = 1000, contigOutputMode = 1;
    // the workflows' --db-mode end (nuclassemble.sh:200-207): nuclassemble-chain --db-mode 1 --db-out DB, and the nested nuclassemble of
    // guidedassemble-chain --nuclassembly-out DB with the nucleotide halves of the multi-parameters (GuidedNuclassembler.cpp:10-14,167-174)
    // createdb-reads and the chains' --single-end 1 (unpaired read files through plasship_createdb): createdb's own defaults (Parameters.cpp: --shuffle 1)
    int singleEnd = 0, shuffle = 1, dbtypeArg = 0, createdbMode = 0, writeLookup = 1; unsigned long long idOffset = 0;
    std::string dbOut, nuclAssemblyOut; int dbMode = 0, numIterationsNucl = 5, kNucl = 22, minAlnLenNucl = 0;
    int clusterMode = 0;                 // clust: Parameters::SET_COVER (not one of kMembers: the dump's lines are pinned as they are)
    float scorePerColThr = 0.0f;         // rescorediagonal-local --score-per-col-thr (our own flag; not one of kMembers either)
    std::string repOut;                  // linclust-ungapped[-prot] --rep-out DB: the representatives' sequence DB (our own flag; not one of kMembers either)
    int maxIterations = 1000;            // clust --max-iterations, read by connected component only (Parameters.cpp:2171; not one of kMembers either)
    std::set<std::string> seen;
};

static std::string fmtNum(const char *fmt, ...) { char b[96]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof(b), fmt, ap); va_end(ap); return b; }
// A value-carrying member of Flags, typed: where the flag table sends a value, and what the dump prints.  PLASSHIP_CLI_DRYRUN=2 prints every one
// of kMembers (declaration order) after the "accepted" line as `flag.<name> <value>`: what the parser made of the command line.  The names are
// part of tests/golden/cli_dryrun_corpus.json and stay as they are, whatever becomes of the struct.
struct Dest {
    enum Type { NONE, INT, FLOAT, DOUBLE, U64, STR } type = NONE;
    int Flags::*i = nullptr; float Flags::*fl = nullptr; double Flags::*d = nullptr; unsigned long long Flags::*u = nullptr; std::string Flags::*s = nullptr;
    Dest() {}
    Dest(int Flags::*p) : type(INT), i(p) {}
    Dest(float Flags::*p) : type(FLOAT), fl(p) {}
    Dest(double Flags::*p) : type(DOUBLE), d(p) {}
    Dest(unsigned long long Flags::*p) : type(U64), u(p) {}
    Dest(std::string Flags::*p) : type(STR), s(p) {}
    void set(Flags &f, const std::string &v) const {
        if (type == INT) f.*i = atoi(v.c_str()); else if (type == FLOAT) f.*fl = strtof(v.c_str(), nullptr); else if (type == DOUBLE) f.*d = strtod(v.c_str(), nullptr);
        else if (type == U64) f.*u = strtoull(v.c_str(), nullptr, 10); else if (type == STR) f.*s = v;
    }
    std::string str(const Flags &f) const {            // the text of the dump and of chain.manifest
        return type == INT ? std::to_string(f.*i) : type == FLOAT ? fmtNum("%.9g", (double) (f.*fl)) : type == DOUBLE ? fmtNum("%.17g", f.*d)
             : type == U64 ? std::to_string(f.*u) : type == STR ? f.*s : std::string();
    }
};
#define M(m) &Flags::m
#define MEMBER(m) {#m, M(m)}
static const struct { const char *name; Dest dest; } kMembers[] = {
    MEMBER(k), MEMBER(alph), MEMBER(kps), MEMBER(hashShift), MEMBER(onlyExt), MEMBER(ignoreMulti), MEMBER(covMode), MEMBER(scaleAA), MEMBER(scaleNucl), MEMBER(covThr),
    MEMBER(seqIdThr), MEMBER(rescoreMode), MEMBER(minAlnLen), MEMBER(seqIdMode), MEMBER(addBt), MEMBER(addSelf), MEMBER(keepTarget), MEMBER(wrapped), MEMBER(filterHits),
    MEMBER(sortResults), MEMBER(evalThr), MEMBER(maxSeqLen), MEMBER(gapOpenNucl), MEMBER(gapExtendNucl), MEMBER(chopCycle), MEMBER(orfMin), MEMBER(orfMax), MEMBER(orfGaps),
    MEMBER(contigStart), MEMBER(contigEnd), MEMBER(orfStart), MEMBER(fwdFrames), MEMBER(revFrames), MEMBER(translationTable), MEMBER(translate), MEMBER(allStarts),
    MEMBER(addOrfStop), MEMBER(preserveKeys), MEMBER(takeLarger), MEMBER(numIterations), MEMBER(fromReads), MEMBER(resume), MEMBER(writeIntermediate), MEMBER(seqIdThrNucl),
    MEMBER(fastaOut), MEMBER(filterProteins), MEMBER(minContigLen), MEMBER(contigOutputMode), MEMBER(singleEnd), MEMBER(shuffle), MEMBER(dbtypeArg), MEMBER(createdbMode),
    MEMBER(writeLookup), MEMBER(idOffset), MEMBER(dbOut), MEMBER(nuclAssemblyOut), MEMBER(dbMode), MEMBER(numIterationsNucl), MEMBER(kNucl), MEMBER(minAlnLenNucl),
};

// Exit codes beyond EXIT_SUCCESS / EXIT_FAILURE: a request that is well-formed for the REFERENCE module but lies
// outside what the GPU path implements (--rescore-mode 0, --wrapped-scoring 1, masking, spaced k-mers, automatic -k, a module that is not
// part of the hot path, PLASSHIP_ERR_UNSUPPORTED from the library) ends with EXIT_UNSUPPORTED before anything is written, so that a
// wrapper can hand exactly that call to the reference binary: `linclust` at the end of `penguin guided_nuclassemble` calls
// `rescorediagonal --rescore-mode 0 --wrapped-scoring 1` (lib/mmseqs/data/workflow/linclust.sh:30) through the same $MMSEQS.
// EXIT_DRYRUN_ACCEPTED: with PLASSHIP_CLI_DRYRUN=1 the command line is parsed and validated, nothing is read or computed (no GPU needed) —
// what tools/workflow_dropin_check.sh uses to exercise the routing of every call the unmodified workflow scripts make.  PLASSHIP_CLI_DRYRUN=2
// adds the parsed values to an accepted call's output (kMembers above): what tests/test_cli_dryrun_corpus.py pins the parser with.
enum { EXIT_UNSUPPORTED = 95, EXIT_DRYRUN_ACCEPTED = 96 };
static int g_lastRc = 0;
static bool g_wrote = false;             // an output DB of this call exists on disk (a completed *_write): exit code 95 would make a wrapper re-run the call over it
static inline int K(int rc) { g_lastRc = rc; return rc; }
static inline int KW(int rc) { g_lastRc = rc; if (rc == 0) g_wrote = true; return rc; }      // K() for the calls that write a DB
static int unsupported(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfprintf(stdout, fmt, ap); va_end(ap);
    fprintf(stdout, "plass-hip: outside the GPU hot path, exit code %d (nothing was written)\n", (int) EXIT_UNSUPPORTED);
    return EXIT_UNSUPPORTED;
}
static int fail(const char *what) {
    fprintf(stdout, "%s: %s\n", what, plasship_last_error());
    if (g_lastRc == PLASSHIP_ERR_UNSUPPORTED && !g_wrote) { fprintf(stdout, "plass-hip: outside the GPU hot path, exit code %d (nothing was written)\n", (int) EXIT_UNSUPPORTED); return EXIT_UNSUPPORTED; }
    // (an "unsupported" that arrives after an output DB of this call was written is an ordinary failure: the files stay as they are and no wrapper
    //  should run the reference over them — ADVICE r5)
    if (g_lastRc == PLASSHIP_ERR_UNSUPPORTED) fprintf(stdout, "plass-hip: part of the output was already written; exit code %d, not %d\n", (int) EXIT_FAILURE, (int) EXIT_UNSUPPORTED);
    return EXIT_FAILURE;
}
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static bool isFile(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
static bool existsAlready(const std::string &p) {         // the workflows' OUT_FILE check (data/assemble.sh:23, nuclassemble.sh:69, guidedNuclAssemble.sh:24)
    struct stat st; const bool there = stat(p.c_str(), &st) == 0;
    if (there) fprintf(stdout, "%s exists already!\n", p.c_str());
    return there;
}
// the database type in <db>.dbtype; -1: the file is not there or too short (a DB that does not exist yet: a dry run on names only)
static int probeDbtype(const std::string &db) {
    unsigned ty = 0; int dbtype = -1;
    if (FILE *ft = fopen((db + ".dbtype").c_str(), "rb")) { if (fread(&ty, 4, 1, ft) == 1) dbtype = (int) (ty & 0x3FFFFFFFu); fclose(ft); }
    return dbtype;
}
static int dbtypeOf(const plasship_seqdb *db) { int t = -1; plasship_seqdb_info(db, nullptr, nullptr, nullptr, &t, nullptr); return t; }
static std::vector<const char *> cstrs(const std::vector<std::string> &v) { std::vector<const char *> p; for (const std::string &s : v) p.push_back(s.c_str()); return p; }

// An owning handle of the library: freed with the context it was made on when it goes out of scope, on every path; ownership moves.
template <class T, void (*Free)(plasship_ctx *, T *)> struct Handle {
    plasship_ctx *ctx; T *p = nullptr;
    explicit Handle(plasship_ctx *c) : ctx(c) {}
    Handle(Handle &&o) : ctx(o.ctx), p(o.p) { o.p = nullptr; }
    Handle &operator=(Handle &&o) { if (this != &o) { reset(); ctx = o.ctx; p = o.p; o.p = nullptr; } return *this; }
    ~Handle() { reset(); }
    void reset() { if (p) Free(ctx, p); p = nullptr; }
    T **out() { reset(); return &p; }                      // for the library's `T **out` arguments
    operator T *() const { return p; }
};
typedef Handle<plasship_seqdb, plasship_seqdb_free> SeqDb; typedef Handle<plasship_orfhdr, plasship_orfhdr_free> OrfHdr;
typedef Handle<plasship_cands, plasship_cands_free> Cands; typedef Handle<plasship_alns, plasship_alns_free> Alns;
typedef Handle<plasship_clusters, plasship_clusters_free> Clusters; typedef Handle<plasship_merged, plasship_merged_free> Merged;

// ---- the modules: one bit each, so that a flag states its owners as a mask ----
enum : unsigned {
    KMERMATCHER = 1u << 0, RESCOREDIAGONAL = 1u << 1, ASSEMBLERESULTS = 1u << 2, NUCLASSEMBLERESULTS = 1u << 3, GUIDEDASSEMBLERESULTS = 1u << 4, PROTEINALN2NUCL = 1u << 5,
    FINDASSEMBLYSTART = 1u << 6, CYCLECHECK = 1u << 7, EXTRACTORFS = 1u << 8, TRANSLATENUCS = 1u << 9, CONCATDBS = 1u << 10, ASSEMBLE_CHAIN = 1u << 11,
    NUCLASSEMBLE_CHAIN = 1u << 12, GUIDEDASSEMBLE_CHAIN = 1u << 13, CREATEDB_READS = 1u << 14, MERGEREADS = 1u << 15, RESCOREDIAGONAL_HAMMING = 1u << 16,
    ANY_ASSEMBLERESULTS = ASSEMBLERESULTS | NUCLASSEMBLERESULTS | GUIDEDASSEMBLERESULTS, CHAINS = ASSEMBLE_CHAIN | NUCLASSEMBLE_CHAIN | GUIDEDASSEMBLE_CHAIN,
    CLUST_GREEDY = 1u << 17, LINCLUST_PRE = 1u << 18, RESCOREDIAGONAL_LOCAL = 1u << 19, MERGECLUSTERS_GREEDY = 1u << 20, LINCLUST_UNGAPPED = 1u << 21,
    RESCOREDIAGONAL_SUBST = 1u << 22, LINCLUST_UNGAPPED_PROT = 1u << 23, CLUST_REPSEQ = 1u << 24, CLUST_CONNECTED = 1u << 25,
    EXTRACTORFS_GENCODE = 1u << 26, TRANSLATENUCS_GENCODE = 1u << 27,      // (extractorfs' and translatenucs' flag sets)
    ANY_EXTRACTORFS = EXTRACTORFS | EXTRACTORFS_GENCODE, ANY_TRANSLATENUCS = TRANSLATENUCS | TRANSLATENUCS_GENCODE,
    ORF_CHAINS = ASSEMBLE_CHAIN | GUIDEDASSEMBLE_CHAIN,                     // the workflows that translate: they hand the table to both modules
    // (rescorediagonal-hamming, rescorediagonal-local and rescorediagonal-subst take rescorediagonal's flag set, clust-greedy clust's; linclust-pre the union of its three steps',
    //  linclust-ungapped the union of linclust-pre's and rescorediagonal-local's; mergeclusters-greedy has the reference's: --threads, --compressed, -v;
    //  linclust-ungapped-prot has linclust-ungapped's set, clust-repseq result2repseq's: --db-load-mode, --compressed, --threads, -v; clust-connected clust's)
    ANY_LINCLUST_UNGAPPED = LINCLUST_UNGAPPED | LINCLUST_UNGAPPED_PROT,
    ANY_KMERMATCHER = KMERMATCHER | LINCLUST_PRE | ANY_LINCLUST_UNGAPPED,
    ANY_RESCOREDIAGONAL = RESCOREDIAGONAL | RESCOREDIAGONAL_HAMMING | RESCOREDIAGONAL_LOCAL | RESCOREDIAGONAL_SUBST | LINCLUST_PRE | ANY_LINCLUST_UNGAPPED,
    ANY_CLUST = CLUST_GREEDY | CLUST_CONNECTED | LINCLUST_PRE | ANY_LINCLUST_UNGAPPED,
    ALL = 0xFFFFFFFu
};

// ---- the flags: each once, with the modules that own it (its parameter vector in the reference; for the fused drivers the workflow's own),
//      how its value is read and where it goes.  Parsing follows Parameters::parseParameters (Parameters.cpp:1560-1700). ----
// VALUE: atoi / strtof / strtod / strtoull / the string itself, by the member's type.  BOOL: a bool of the reference (typeid(bool)): TRUE/1 | FALSE/0, and a
// missing value toggles the current one (Parameters.cpp:1670-1677).  AA, NUCL: a MultiParam of which this build reads one half ("aa:13,nucl:5"; one value
// sets both halves, MultiParam.cpp:23-39).  BOTH: a MultiParam, the aa half goes to `a`, the nucl half to `b`.  BOTH_GUIDED: BOTH on guidedassemble-chain,
// VALUE (of the whole string) on every other module.  FRAMES: Orf::getFrames, "1,2,3" as a bit mask.  IGNORED: takes a value that cannot influence the
// result.  ZERO / ZERO_BOOL / EMPTY: must be 0 / a BOOL that stays 0 / the empty string, anything else is outside the GPU path (exit code 95).
// CUSTOM: read by its own handler, which returns 0 or the exit code.
enum Kind { VALUE, BOOL, AA, NUCL, BOTH, BOTH_GUIDED, FRAMES, IGNORED, ZERO, ZERO_BOOL, EMPTY, CUSTOM };
struct Flag { const char *name; unsigned owners; Kind kind; Dest a, b; int (*custom)(Flags &f, unsigned mod, const std::string &v); };
static void half(Flags &f, const std::string &v, const char *which, const Dest &d) { std::string t; if (multiParam(v, which, t)) d.set(f, t); }

static int subMatFlag(Flags &, unsigned, const std::string &v) {      // only the matrices the tables were captured from: blosum62.out (amino acids) and nucleotide.out
    std::string aa, nu;
    const bool multi = v.find(':') != std::string::npos, okA = multiParam(v, "aa", aa), okN = multiParam(v, "nucl", nu);
    if (multi ? (okA && baseName(aa) != "blosum62.out") || (okN && baseName(nu) != "nucleotide.out") : baseName(v) != "blosum62.out" && baseName(v) != "nucleotide.out")
        return unsupported("plass-hip: --sub-mat %s is not supported (built for blosum62.out / nucleotide.out)\n", v.c_str());
    return 0;
}
static int minSeqIdFlag(Flags &f, unsigned mod, const std::string &v) {      // the guided chain reads both halves, the other two chains their own, a module the whole value
    if (mod == GUIDEDASSEMBLE_CHAIN) { half(f, v, "aa", &Flags::seqIdThr); half(f, v, "nucl", &Flags::seqIdThrNucl); }
    else if (mod & CHAINS) half(f, v, mod == NUCLASSEMBLE_CHAIN ? "nucl" : "aa", &Flags::seqIdThr);
    else f.seqIdThr = strtof(v.c_str(), nullptr);
    return 0;
}
static int numIterationsFlag(Flags &f, unsigned mod, const std::string &v) {  // the chain's own half (or the whole string); the nucl half is also the nested nuclassemble's count
    std::string t;
    f.numIterations = atoi((multiParam(v, mod == NUCLASSEMBLE_CHAIN ? "nucl" : "aa", t) ? t : v).c_str());
    half(f, v, "nucl", &Flags::numIterationsNucl);
    return 0;
}
static int idOffsetFlag(Flags &f, unsigned mod, const std::string &v) {       // createdb's value; extractorfs' must be 0
    if (mod == CREATEDB_READS) f.idOffset = strtoull(v.c_str(), nullptr, 10);
    else if (atoi(v.c_str()) != 0) return unsupported("%s %s is not supported by plass-hip\n", "--id-offset", v.c_str());
    return 0;
}
static const Flag kFlags[] = {
    {"--threads", ALL, IGNORED}, {"-v", ALL, IGNORED}, {"--compressed", ALL, ZERO},
    // shared by several modules (and the fused drivers, which take the workflows' own flags)
    {"--sub-mat", ANY_KMERMATCHER | ANY_RESCOREDIAGONAL | PROTEINALN2NUCL, CUSTOM, {}, {}, subMatFlag}, {"--alph-size", ANY_KMERMATCHER | CHAINS, AA, M(alph)},
    {"--min-seq-id", ANY_KMERMATCHER | ANY_RESCOREDIAGONAL | ANY_ASSEMBLERESULTS | CHAINS, CUSTOM, {}, {}, minSeqIdFlag}, {"--kmer-per-seq", ANY_KMERMATCHER | CHAINS, VALUE, M(kps)},
    {"--kmer-per-seq-scale", ANY_KMERMATCHER | CHAINS, BOTH, M(scaleAA), M(scaleNucl)}, {"--cov-mode", ANY_KMERMATCHER | ANY_RESCOREDIAGONAL | CHAINS, VALUE, M(covMode)},
    {"-k", ANY_KMERMATCHER | CHAINS, BOTH_GUIDED, M(k), M(kNucl)}, {"-c", ANY_KMERMATCHER | ANY_RESCOREDIAGONAL | CHAINS, VALUE, M(covThr)},
    {"--max-seq-len", ANY_KMERMATCHER | ANY_ASSEMBLERESULTS | CYCLECHECK | CHAINS, VALUE, M(maxSeqLen)}, {"--hash-shift", ANY_KMERMATCHER | CHAINS, VALUE, M(hashShift)},
    {"--ignore-multi-kmer", ANY_KMERMATCHER | CHAINS, BOOL, M(ignoreMulti)}, {"--rescore-mode", ANY_RESCOREDIAGONAL | ANY_ASSEMBLERESULTS | CHAINS, VALUE, M(rescoreMode)},
    {"-e", ANY_RESCOREDIAGONAL | CHAINS, VALUE, M(evalThr)}, {"--min-aln-len", ANY_RESCOREDIAGONAL | CHAINS, BOTH_GUIDED, M(minAlnLen), M(minAlnLenNucl)},
    {"--seq-id-mode", ANY_RESCOREDIAGONAL | CHAINS, VALUE, M(seqIdMode)}, {"--keep-target", ANY_ASSEMBLERESULTS | CHAINS, BOOL, M(keepTarget)},
    {"--chop-cycle", CYCLECHECK | NUCLASSEMBLE_CHAIN | GUIDEDASSEMBLE_CHAIN, BOOL, M(chopCycle)}, {"--translation-table", ANY_EXTRACTORFS | ANY_TRANSLATENUCS | ORF_CHAINS, VALUE, M(translationTable)},
    {"--id-offset", ANY_EXTRACTORFS | CREATEDB_READS, CUSTOM, {}, {}, idOffsetFlag},
    // one module's own
    {"--spaced-kmer-mode", ANY_KMERMATCHER, ZERO}, {"--spaced-kmer-pattern", ANY_KMERMATCHER, EMPTY}, {"--adjust-kmer-len", ANY_KMERMATCHER, ZERO_BOOL}, {"--mask", ANY_KMERMATCHER, ZERO},
    {"--mask-lower-case", ANY_KMERMATCHER, ZERO}, {"--split-memory-limit", ANY_KMERMATCHER, IGNORED}, {"--include-only-extendable", ANY_KMERMATCHER, BOOL, M(onlyExt)},
    {"--wrapped-scoring", ANY_RESCOREDIAGONAL, BOOL, M(wrapped)}, {"--filter-hits", ANY_RESCOREDIAGONAL, BOOL, M(filterHits)}, {"-a", ANY_RESCOREDIAGONAL, BOOL, M(addBt)},
    {"--add-self-matches", ANY_RESCOREDIAGONAL, BOOL, M(addSelf)}, {"--sort-results", ANY_RESCOREDIAGONAL, VALUE, M(sortResults)}, {"--db-load-mode", ANY_RESCOREDIAGONAL | CLUST_REPSEQ, IGNORED},
    {"--score-per-col-thr", RESCOREDIAGONAL_LOCAL | RESCOREDIAGONAL_SUBST | ANY_LINCLUST_UNGAPPED, VALUE, M(scorePerColThr)}, {"--rep-out", ANY_LINCLUST_UNGAPPED, VALUE, M(repOut)},
    {"--cluster-mode", ANY_CLUST, VALUE, M(clusterMode)}, {"--max-iterations", ANY_CLUST, VALUE, M(maxIterations)}, {"--similarity-type", ANY_CLUST, IGNORED},
    {"--gap-open", PROTEINALN2NUCL, NUCL, M(gapOpenNucl)}, {"--gap-extend", PROTEINALN2NUCL, NUCL, M(gapExtendNucl)},
    {"--min-length", ANY_EXTRACTORFS, VALUE, M(orfMin)}, {"--max-length", ANY_EXTRACTORFS, VALUE, M(orfMax)}, {"--max-gaps", ANY_EXTRACTORFS, VALUE, M(orfGaps)},
    {"--contig-start-mode", ANY_EXTRACTORFS, VALUE, M(contigStart)}, {"--contig-end-mode", ANY_EXTRACTORFS, VALUE, M(contigEnd)}, {"--orf-start-mode", ANY_EXTRACTORFS, VALUE, M(orfStart)},
    {"--forward-frames", ANY_EXTRACTORFS, FRAMES, M(fwdFrames)}, {"--reverse-frames", ANY_EXTRACTORFS, FRAMES, M(revFrames)}, {"--translate", ANY_EXTRACTORFS, VALUE, M(translate)},
    {"--use-all-table-starts", ANY_EXTRACTORFS | ORF_CHAINS, BOOL, M(allStarts)}, {"--create-lookup", ANY_EXTRACTORFS, ZERO}, {"--add-orf-stop", ANY_TRANSLATENUCS, BOOL, M(addOrfStop)},
    {"--preserve-keys", CONCATDBS, BOOL, M(preserveKeys)}, {"--take-larger-entry", CONCATDBS, BOOL, M(takeLarger)},
    {"--shuffle", CREATEDB_READS, BOOL, M(shuffle)}, {"--dbtype", CREATEDB_READS, VALUE, M(dbtypeArg)}, {"--createdb-mode", CREATEDB_READS, VALUE, M(createdbMode)},
    {"--write-lookup", CREATEDB_READS, VALUE, M(writeLookup)},
    // the fused drivers only.  (--protein-filter-threshold is filternoncoding's: only read by the step --filter-proteins 1 runs.  --nuclassembly-out DB: the
    // nuclassemble of data/guidedNuclAssemble.sh:135-170 behind the guided loop, with the nucleotide workflow's own flags)
    {"--num-iterations", CHAINS, CUSTOM, {}, {}, numIterationsFlag}, {"--write-intermediate", CHAINS, VALUE, M(writeIntermediate)}, {"--from-reads", CHAINS, VALUE, M(fromReads)},
    {"--resume", CHAINS, VALUE, M(resume)}, {"--single-end", CHAINS, VALUE, M(singleEnd)}, {"--fasta-out", ASSEMBLE_CHAIN | NUCLASSEMBLE_CHAIN, VALUE, M(fastaOut)},
    {"--filter-proteins", ASSEMBLE_CHAIN, VALUE, M(filterProteins)}, {"--protein-filter-threshold", ASSEMBLE_CHAIN, IGNORED},
    {"--min-contig-len", NUCLASSEMBLE_CHAIN | GUIDEDASSEMBLE_CHAIN, VALUE, M(minContigLen)}, {"--contig-output-mode", NUCLASSEMBLE_CHAIN | GUIDEDASSEMBLE_CHAIN, VALUE, M(contigOutputMode)},
    {"--db-mode", NUCLASSEMBLE_CHAIN, BOOL, M(dbMode)}, {"--db-out", NUCLASSEMBLE_CHAIN, VALUE, M(dbOut)}, {"--nuclassembly-out", GUIDEDASSEMBLE_CHAIN, VALUE, M(nuclAssemblyOut)},
};
static int parseBool(const std::string &v) { return v == "1" || v == "TRUE" || v == "true" ? 1 : v == "0" || v == "FALSE" || v == "false" ? 0 : -1; }    // Parameters::parseBool; -1: neither
// one flag and its value (haveValue false: a bool without one) -> 0, or the exit code
static int applyFlag(const Flag &fl, Flags &f, unsigned mod, const std::string &v, bool haveValue) {
    auto setBool = [&](int &field) {
        const int b = haveValue ? parseBool(v) : !field;
        if (b < 0) fprintf(stdout, "Error in argument %s\n", fl.name); else field = b;
        return b >= 0;
    };
    int zero = 0;
    switch (fl.kind) {
        case VALUE: fl.a.set(f, v); break;
        case BOOL: if (!setBool(f.*fl.a.i)) return EXIT_FAILURE; break;
        case AA: half(f, v, "aa", fl.a); break;
        case NUCL: half(f, v, "nucl", fl.a); break;
        case BOTH_GUIDED: if (mod != GUIDEDASSEMBLE_CHAIN) { fl.a.set(f, v); break; }
            [[fallthrough]];
        case BOTH: half(f, v, "aa", fl.a); half(f, v, "nucl", fl.b); break;
        case FRAMES: { bool ok; f.*fl.a.i = frameMask(v, ok);
            if (!ok) { fprintf(stdout, "Error in argument %s\n", fl.name); return EXIT_FAILURE; }
            break; }
        case IGNORED: break;
        case ZERO: if (atoi(v.c_str()) != 0) return unsupported("%s %s is not supported by plass-hip\n", fl.name, v.c_str()); break;
        case ZERO_BOOL: if (!setBool(zero) || zero) return zero ? unsupported("%s is not supported by plass-hip\n", fl.name) : EXIT_FAILURE; break;
        case EMPTY: if (!v.empty()) return unsupported("%s is not supported by plass-hip\n", fl.name); break;
        case CUSTOM: return fl.custom(f, mod, v);
    }
    return 0;
}

// ---- the parameter structs of the library from the flags, each written once: the modules use them as they are, the fused drivers state
//      where they differ ----
static plasship_kmermatch_params kmermatchParams(const Flags &f, float scale) {      // scale: --kmer-per-seq-scale for the DB's alphabet
    plasship_kmermatch_params p = {};
    p.kmer_size = f.k; p.alphabet_size = f.alph; p.kmers_per_seq = f.kps; p.kmers_per_seq_scale = scale; p.hash_shift = f.hashShift;
    p.include_only_extendable = f.onlyExt; p.ignore_multi_kmer = f.ignoreMulti; p.cov_mode = f.covMode; p.cov_thr = f.covThr;
    return p;
}
static plasship_rescore_params rescoreParams(const Flags &f) {
    plasship_rescore_params p = {};
    p.rescore_mode = f.rescoreMode; p.eval_thr = f.evalThr; p.seq_id_thr = f.seqIdThr; p.cov_mode = f.covMode; p.cov_thr = f.covThr;
    p.min_aln_len = f.minAlnLen; p.seq_id_mode = f.seqIdMode; p.add_backtrace = f.addBt; p.include_identity = f.addSelf;
    return p;
}
static plasship_hamming_params hammingParams(const Flags &f) {
    plasship_hamming_params p = {};
    p.wrapped = f.wrapped; p.seq_id_thr = f.seqIdThr; p.seq_id_mode = f.seqIdMode; p.cov_mode = f.covMode; p.cov_thr = f.covThr; p.min_aln_len = f.minAlnLen; p.eval_thr = f.evalThr;
    return p;
}
static plasship_local_params localParams(const Flags &f) {
    plasship_local_params p = {};
    p.eval_thr = f.evalThr; p.seq_id_thr = f.seqIdThr; p.seq_id_mode = f.seqIdMode; p.cov_thr = f.covThr; p.cov_mode = f.covMode; p.min_aln_len = f.minAlnLen;
    p.add_backtrace = f.addBt; p.score_per_col_thr = f.filterHits ? f.scorePerColThr : NAN;
    return p;
}
static plasship_subst_params substParams(const Flags &f) {
    plasship_subst_params p = {};
    p.eval_thr = f.evalThr; p.seq_id_thr = f.seqIdThr; p.cov_thr = f.covThr; p.cov_mode = f.covMode; p.min_aln_len = f.minAlnLen;
    p.score_per_col_thr = f.filterHits ? f.scorePerColThr : NAN;
    return p;
}
static plasship_assemble_params assembleParams(const Flags &f) {
    plasship_assemble_params p = {}; p.seq_id_thr = f.seqIdThr; p.max_seq_len = f.maxSeqLen; p.keep_target = f.keepTarget; p.rescore_mode = f.rescoreMode;
    return p;
}
static plasship_aln2nucl_params aln2nuclParams(const Flags &f) { plasship_aln2nucl_params p; p.gap_open = f.gapOpenNucl; p.gap_extend = f.gapExtendNucl; return p; }
static plasship_cyclecheck_params cyclecheckParams(const Flags &f) { plasship_cyclecheck_params p; p.max_seq_len = f.maxSeqLen; p.chop_cycle = f.chopCycle; return p; }
static plasship_orf_params orfParams(const Flags &f) {
    plasship_orf_params p; memset(&p, 0, sizeof(p));
    p.min_length = f.orfMin; p.max_length = f.orfMax; p.max_gaps = f.orfGaps; p.contig_start_mode = f.contigStart; p.contig_end_mode = f.contigEnd;
    p.orf_start_mode = f.orfStart; p.forward_frames = f.fwdFrames; p.reverse_frames = f.revFrames; p.translation_table = f.translationTable;
    p.translate = f.translate; p.use_all_table_starts = f.allStarts; p.max_seq_len = f.maxSeqLen;
    return p;
}


// ---- the iteration loop of a workflow script (data/assemble.sh:85-156, nuclassemble.sh:95-137, guidedNuclAssemble.sh:77-126) with every DB of
//      the loop resident in HBM.  One function for the three drivers and for the nuclassemble that guidedassemble-chain --nuclassembly-out
//      runs on the merged DB (guidedNuclAssemble.sh:167-170). ----
enum ChainKind { CHAIN_PROTEIN, CHAIN_NUCL, CHAIN_GUIDED };
struct ChainLoop {
    plasship_ctx *ctx; const char *name = ""; ChainKind kind = CHAIN_PROTEIN;
    int numIterations = 1, startIteration = 0;
    // what the loop hands to the library (kp.hash_shift and kp.include_only_extendable: see the loop); np on the guided chain, cp on nucleotides
    plasship_kmermatch_params kp; plasship_rescore_params rp; plasship_assemble_params ap; plasship_aln2nucl_params np; plasship_cyclecheck_params cp;
    bool keepForTail = false;            // keep SOURCE and every iteration's circular contigs: a tail follows
    std::string cyclePrefix;             // nucleotide: circular contigs of iteration i are written to <cyclePrefix><i> ("": they are not)
    std::string intermediateName;        // --write-intermediate: "assembly_" / "assembly_nucl_" ("": nothing is written)
    bool writeLastIntermediate = false;  // --resume 1: the last iteration's DB is a resume point too (a finished run can be extended)
    std::function<int()> joinWriter; std::function<void(const plasship_seqdb *, const std::string &)> writeAsync;
    // in: the DB(s) iteration startIteration starts from; out: the last iteration's
    SeqDb db, aa;
    // keepForTail: SOURCE of the tail — the DB the loop starts from (the reads; the guided chain's nucl_6f_start_long; the fragments before
    // findassemblystart) — and PREV_CYCLE_ALL (empty: no circular contig).  A loop that starts at iteration 0 sets both; one that starts
    // later (--resume 1) is handed what the iterations before startIteration would have left here
    SeqDb source, cycAll;
    unsigned long long overlaps = 0; double kernelMs = 0, tStart = 0;
    ChainLoop(plasship_ctx *c, const char *n, ChainKind k, const Flags &f) : ctx(c), name(n), kind(k), db(c), aa(c), source(c), cycAll(c) {
        kp = kmermatchParams(f, k == CHAIN_NUCL ? f.scaleNucl : f.scaleAA); rp = rescoreParams(f); ap = assembleParams(f); np = aln2nuclParams(f); cp = cyclecheckParams(f);
    }
};
static int runChainLoop(ChainLoop &L) {
    plasship_ctx *ctx = L.ctx;
    const bool prot = L.kind == CHAIN_PROTEIN, nuc = L.kind == CHAIN_NUCL, gd = L.kind == CHAIN_GUIDED;
    SeqDb &db = L.db, &aa = L.aa;
    for (int it = L.startIteration; it < L.numIterations; it++) {
        plasship_kmermatch_params kp = L.kp;
        // plass assemble: --hash-shift grows with every second iteration, iteration 0 keeps non-extendable matches (Assembler.cpp:99-110)
        // (67, 68, 68, 69, …: a function of the iteration's index, wherever this loop starts)
        if (prot) { kp.hash_shift = L.kp.hash_shift + (it + 1) / 2; kp.include_only_extendable = it > 0; } else kp.include_only_extendable = 1;
        SeqDb next(ctx), nextAa(ctx); plasship_kmermatch_stats ks; plasship_rescore_stats rs; plasship_assemble_stats as;
        {
            const plasship_seqdb *q = gd ? aa.p : db.p;
            Cands c(ctx); Alns al(ctx);
            if (K(plasship_kmermatch(ctx, q, &kp, c.out(), &ks)) || K(plasship_rescore(ctx, q, q, c, &L.rp, al.out(), &rs))) return fail(L.name);
            if (prot && it == 0) {         // data/assemble.sh:110-141: findassemblystart, then k-mer matching and re-scoring again on the corrected sequences
                SeqDb corr(ctx); plasship_findstart_stats fs;
                if (K(plasship_find_assembly_start(ctx, db, al, corr.out(), &fs))) return fail(L.name);
                al.reset(); c.reset();
                if (L.keepForTail) L.source = std::move(db);      // SOURCE of the tail: aa_6f_start_long, before the correction
                db = std::move(corr); q = db.p;
                if (K(plasship_kmermatch(ctx, q, &kp, c.out(), &ks)) || K(plasship_rescore(ctx, q, q, c, &L.rp, al.out(), &rs))) return fail(L.name);
            }
            L.overlaps += ks.n_candidates; L.kernelMs += ks.ms_extract + ks.ms_sort1 + ks.ms_group + ks.ms_sort2 + ks.ms_reduce + rs.ms_kernel;
            if (gd) {
                Alns na(ctx); plasship_aln2nucl_stats ns;
                if (K(plasship_aln2nucl(ctx, db, db, aa, aa, al, &L.np, na.out(), &ns)) || K(plasship_guided_assemble(ctx, db, aa, na, &L.ap, next.out(), nextAa.out(), &as))) return fail(L.name);
            } else if (K(plasship_assemble(ctx, db, al, &L.ap, next.out(), &as))) return fail(L.name);
            L.kernelMs += as.ms_kernel;
        }
        if (L.joinWriter && L.joinWriter()) return EXIT_FAILURE;   // the writer read `db`, which goes now (the caller's joinWriter prints the message)
        if (L.keepForTail && !prot && !L.source) L.source = std::move(db);      // SOURCE of the tail: the DB the loop started from
        db = std::move(next); aa = std::move(nextAa);
        if (nuc) {     // data/nuclassemble.sh:19-61,132: circular contigs leave the loop, the rest goes on
            SeqDb cyc(ctx), rest(ctx); plasship_cyclecheck_stats cs;
            if (K(plasship_cyclecheck(ctx, db, &L.cp, cyc.out(), rest.out(), &cs))) return fail(L.name);
            if (cs.n_cyclic && !L.cyclePrefix.empty() && KW(plasship_seqdb_write(ctx, cyc, (L.cyclePrefix + std::to_string(it)).c_str()))) return fail(L.name);
            if (L.keepForTail && cs.n_cyclic) {       // PREV_CYCLE_ALL: every iteration's circular contigs (nuclassemble.sh:35-41, concatdbs --preserve-keys)
                if (!L.cycAll) L.cycAll = std::move(cyc);
                else { SeqDb u(ctx); if (K(plasship_seqdb_concat_keys(ctx, L.cycAll, cyc, 1, u.out()))) return fail(L.name); L.cycAll = std::move(u); }
            }
            cyc.reset(); db = std::move(rest);
        }
        fprintf(stdout, "iteration %d: candidates %llu verified %llu extended %llu (%.3f s since the DB was read)\n", it, (unsigned long long) ks.n_candidates, (unsigned long long) rs.n_accepted, (unsigned long long) as.n_extended, now() - L.tStart);
        if ((it + 1 < L.numIterations || L.writeLastIntermediate) && L.writeAsync && !L.intermediateName.empty()) L.writeAsync(db, L.intermediateName + std::to_string(it));
    }
    return EXIT_SUCCESS;
}
// ---- the workflows' tail on the last DB of a loop (data/assemble.sh:159-201, nuclassemble.sh:138-207): RESULT, the `_only_assembled` selection,
//      then FASTA (fastaOut) or, in db-mode, the DB of the selected contigs and its cycle index (dbOut).  Takes the loop's source and cycAll over. ----
static int chainTail(plasship_ctx *ctx, const char *name, bool nuc, const plasship_seqdb *db, SeqDb &&sourceOfLoop, SeqDb &&cycAllOfLoop, const Flags &f,
                     const std::string &fastaOut, const std::string &dbOut) {
    SeqDb source = std::move(sourceOfLoop), cycAll = std::move(cycAllOfLoop), merged(ctx), sel(ctx);
    // RESULT: the last assembly, or (nucleotide, circular contigs found) the non-circular rest + every circular contig (nuclassemble.sh:140-148)
    const plasship_seqdb *result = db;
    if (cycAll) { if (K(plasship_seqdb_concat_keys(ctx, db, cycAll, 1, merged.out()))) return fail(name); result = merged; }
    plasship_select_params sp = {}; sp.mode = nuc ? PLASSHIP_SELECT_NUCLEOTIDE : PLASSHIP_SELECT_PROTEIN; sp.only_extended = f.contigOutputMode == 1; sp.min_contig_len = f.minContigLen;
    plasship_select_stats ss;
    if (!source) { fprintf(stdout, "%s: the tail needs the fragment DB before findassemblystart\n", name); return EXIT_FAILURE; }
    if (K(plasship_select_contigs(ctx, result, source, cycAll, &sp, sel.out(), &ss))) return fail(name);
    size_t nResult = 0; plasship_seqdb_info(result, &nResult, nullptr, nullptr, nullptr, nullptr);
    if (!fastaOut.empty()) {
        plasship_fasta_stats fs;
        if (KW(plasship_fasta_write(ctx, sel, cycAll, fastaOut.c_str(), &fs))) return fail(name);
        fprintf(stdout, "fasta: %llu of %zu contigs selected (S1 only %llu, S2 only %llu, both %llu, circular %llu), %llu bytes | select %.3f ms, format %.3f ms, file %.3f s\n",
                (unsigned long long) ss.n_selected, nResult, (unsigned long long) ss.n_s1_only, (unsigned long long) ss.n_s2_only,
                (unsigned long long) ss.n_both, (unsigned long long) ss.n_cycle, (unsigned long long) fs.bytes, ss.ms_kernel, fs.ms_kernel, fs.ms_total * 1e-3);
    } else {
        plasship_subdb_stats ds;
        if (KW(plasship_subdb_write(ctx, sel, cycAll, dbOut.c_str(), &ds))) return fail(name);
        fprintf(stdout, "db-mode: %llu of %zu contigs selected (circular %llu), %llu bytes | select %.3f ms, gather %.3f ms, files %.3f s\n",
                (unsigned long long) ss.n_selected, nResult, (unsigned long long) ds.n_cycle, (unsigned long long) ds.bytes, ss.ms_kernel, ds.ms_kernel, ds.ms_total * 1e-3);
    }
    return EXIT_SUCCESS;
}

// ---- --resume 1: the resume points --write-intermediate DIR leaves (DIR/assembly_<i> + DIR/assembly_<i>.done, data/assemble.sh:147) and
//      DIR/chain.manifest, the parameters and the input they were computed with ----
// the highest i < numIterations whose sentinel and DB files exist (the sentinel is touched after the DB is complete); -1: none
static int resumePoint(const std::string &dir, const std::string &name, int numIterations) {
    for (int i = numIterations - 1; i >= 0; i--) {
        const std::string p = dir + "/" + name + std::to_string(i);
        if (isFile(p + ".done") && isFile(p) && isFile(p + ".index") && isFile(p + ".dbtype")) return i;
    }
    return -1;
}
typedef std::vector<std::pair<std::string, std::string>> Manifest;
// what a continuation must share with the run that wrote the resume points: the module, every parameter the loop's result depends on (keyed
// by its flag) and the input files.  Not --num-iterations, the outputs or the tail's flags: those may differ.
static Manifest chainManifest(const std::string &mod, const Flags &f, const std::vector<std::string> &inputs) {
    Manifest m;
    m.emplace_back("module", mod);
    static const struct { const char *key; Dest dest; } params[] = {
        {"-k", M(k)}, {"--alph-size", M(alph)}, {"--kmer-per-seq", M(kps)}, {"--kmer-per-seq-scale", {}}, {"--hash-shift", M(hashShift)}, {"--min-seq-id", M(seqIdThr)}, {"-e", M(evalThr)},
        {"-c", M(covThr)}, {"--cov-mode", M(covMode)}, {"--min-aln-len", M(minAlnLen)}, {"--seq-id-mode", M(seqIdMode)}, {"--rescore-mode", M(rescoreMode)},
        {"--ignore-multi-kmer", M(ignoreMulti)}, {"--include-only-extendable", M(onlyExt)}, {"--keep-target", M(keepTarget)}, {"--max-seq-len", M(maxSeqLen)},
        {"--chop-cycle", M(chopCycle)}, {"--from-reads", M(fromReads)}, {"--single-end", M(singleEnd)},
        {"--translation-table", M(translationTable)}, {"--use-all-table-starts", M(allStarts)},
    };
    const Dest scale = mod == "nuclassemble-chain" ? M(scaleNucl) : M(scaleAA);      // (the half of --kmer-per-seq-scale the chain's alphabet reads)
    for (const auto &p : params) m.emplace_back(p.key, (p.dest.type == Dest::NONE ? scale : p.dest).str(f));
    m.emplace_back("inputs", std::to_string(inputs.size()));
    for (size_t i = 0; i < inputs.size(); i++) {
        const std::string key = "input." + std::to_string(i);
        char *rp = realpath(inputs[i].c_str(), nullptr);
        m.emplace_back(key + ".path", rp ? rp : inputs[i].c_str()); free(rp);
        struct stat st; const bool have = stat(inputs[i].c_str(), &st) == 0;
        m.emplace_back(key + ".size", have ? std::to_string((long long) st.st_size) : "-1");
        m.emplace_back(key + ".mtime", have ? fmtNum("%lld.%09ld", (long long) st.st_mtim.tv_sec, (long) st.st_mtim.tv_nsec) : "-1");
    }
    return m;
}
static bool writeManifest(const std::string &path, const Manifest &m) {
    const std::string tmp = path + ".tmp";
    FILE *fd = fopen(tmp.c_str(), "w"); if (!fd) return false;
    bool ok = true;
    for (const auto &kv : m) ok &= fprintf(fd, "%s %s\n", kv.first.c_str(), kv.second.c_str()) > 0;
    ok &= fclose(fd) == 0;
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); return false; }
    return true;
}
// the first key of `m` that the manifest file does not hold with the same value ("": none).  A line is "key value", the value runs to its end.
static std::string manifestDiffers(const std::string &path, const Manifest &m, std::string &inFile) {
    std::map<std::string, std::string> have;
    FILE *fd = fopen(path.c_str(), "r"); if (!fd) return m.front().first;
    char line[PATH_MAX + 128];
    while (fgets(line, sizeof(line), fd)) {
        std::string l = line; while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
        const size_t sp = l.find(' ');
        if (!l.empty()) have[l.substr(0, sp)] = sp == std::string::npos ? std::string() : l.substr(sp + 1);
    }
    fclose(fd);
    for (const auto &kv : m) {
        const auto it = have.find(kv.first);
        if (it == have.end()) { inFile = "(missing)"; return kv.first; }
        if (it->second != kv.second) { inFile = it->second; return kv.first; }
    }
    return std::string();
}

// ---- one call: the module, what the command line said, and what the validation before the dry-run exit worked out ----
struct Module;
struct Call {
    const Module *m = nullptr; Flags f; std::vector<std::string> pos;
    std::vector<std::string> readFiles;  // mergereads, createdb-reads, a chain started from read files: the positionals before the output(s)
    int resumeFrom = -1; Manifest manifest;      // --resume 1: the iteration to go on behind (-1: none), and what chain.manifest has to hold
    plasship_ctx *ctx = nullptr; double t0 = 0;
};
struct Module {
    const char *name; unsigned id;
    size_t nPos; const char *usage;      // after the context exists: this many positionals (or read files), else `usage` and EXIT_FAILURE; 0: validate() looked
    void (*defaults)(Flags &);           // where the module's defaults differ from Parameters::setDefaults (nullptr: nowhere)
    int (*validate)(Call &);             // everything that is refused before the dry-run exit and before anything is read: 0, or the exit code
    int (*run)(Call &);
};
static size_t nChainOut(const Call &c) { return c.m->id == GUIDEDASSEMBLE_CHAIN ? 2 : 1; }

// mergereads, createdb-reads and the chains started from read files: the inputs KSeqFactory reads without this path's parser (KSeqWrapper.cpp:160-195)
// are refused by name here; what only the contents show (FASTA for mergereads, multi-line records, quality bytes >= 128) comes back from the
// library as PLASSHIP_ERR_UNSUPPORTED before anything is written
static int takeReadFiles(Call &c, size_t nOutputs) {        // every positional before the output(s)
    c.readFiles.assign(c.pos.begin(), c.pos.end() - nOutputs);
    for (const std::string &q : c.readFiles) {
        if (q == "stdin") return unsupported("plass-hip %s: reading stdin is left to the reference\n", c.m->name);
        if (q.size() >= 4 && q.compare(q.size() - 4, 4, ".bz2") == 0) return unsupported("plass-hip %s: bzip2 input (%s) is left to the reference\n", c.m->name, q.c_str());
    }
    return 0;
}
// an id outside TranslateNucl.h:82-108 ends the reference ("Invalid translation table selected!", TranslateNucl.h:242-245): an error of the call here too
static int validateGencode(Call &c) {
    if (plasship_gencode_info(c.f.translationTable, nullptr, nullptr) == 0) return 0;
    fprintf(stdout, "Invalid translation table selected! (--translation-table %d)\n", c.f.translationTable);
    return EXIT_FAILURE;
}
static int validateKmermatcher(Call &c) {
    // the module's own defaults for these two are "choose automatically" (k = 0: from the DB size, kmermatcher.cpp:607-613; --kmer-per-seq 0): not
    // reproduced — every workflow passes them.  (The reference's module default is spaced k-mers and masking ON unless told otherwise; the workflows
    // run with both off, setLinearFilterDefault turns them off for kmermatcher itself.)
    return c.f.k <= 0 || c.f.kps <= 0 ? unsupported("plass-hip kmermatcher: -k and --kmer-per-seq must be given (the automatic choice of the reference is not implemented)\n") : 0;
}
static int validateRescorediagonal(Call &c) {
    if (c.f.wrapped || c.f.filterHits || c.f.sortResults) return unsupported("--wrapped-scoring/--filter-hits/--sort-results are not supported by plass-hip\n");
    return c.f.rescoreMode != 3 ? unsupported("plass-hip rescorediagonal: --rescore-mode %d is not part of the GPU path (the assembly workflows use mode 3)\n", c.f.rescoreMode) : 0;
}
// rescorediagonal-hamming (our own name: the row above keeps its answers): linclust's Hamming pre-clustering call, lib/mmseqs/data/workflow/linclust.sh:30
static int validateRescoreHamming(Call &c) {
    if (c.f.filterHits || c.f.sortResults > 0) return unsupported("plass-hip rescorediagonal-hamming: --filter-hits 1 / --sort-results are not part of the GPU path\n");
    if (c.f.rescoreMode != 0) return unsupported("plass-hip rescorediagonal-hamming: --rescore-mode %d is not this module's (0, the Hamming score, only)\n", c.f.rescoreMode);
    return c.pos.size() == 4 && c.pos[0] != c.pos[1] ? unsupported("plass-hip rescorediagonal-hamming: separate query and target DBs are not part of the GPU path (linclust uses one DB)\n") : 0;
}
// rescorediagonal-local (our own name: `rescorediagonal --rescore-mode 2` keeps its answer): linclust's alignment step with --alignment-mode 4,
// lib/mmseqs/src/workflow/Linclust.cpp:86-129.  --filter-hits 1 compares the score per column with a threshold the reference reads from a table in
// its binary (rescorediagonal.cpp:20-43,95-105); that table is not part of this build, so the threshold comes with our own --score-per-col-thr
static int validateRescoreLocal(Call &c) {
    if (c.f.rescoreMode != 2) return unsupported("plass-hip rescorediagonal-local: --rescore-mode %d is not this module's (2, the local ungapped alignment, only)\n", c.f.rescoreMode);
    if (c.f.wrapped || c.f.sortResults > 0) return unsupported("plass-hip rescorediagonal-local: --wrapped-scoring 1 / --sort-results are not part of the GPU path\n");
    if (c.f.filterHits && !c.f.seen.count("--score-per-col-thr"))
        return unsupported("plass-hip rescorediagonal-local: --filter-hits 1 needs --score-per-col-thr X (the reference's threshold table is not part of this build)\n");
    return c.pos.size() == 4 && c.pos[0] != c.pos[1] ? unsupported("plass-hip rescorediagonal-local: separate query and target DBs are not part of the GPU path (linclust uses one DB)\n") : 0;
}
// rescorediagonal-subst (our own name: `rescorediagonal --rescore-mode 1` keeps its answer): the filter step linclust runs on amino-acid DBs,
// lib/mmseqs/data/workflow/linclust.sh:59-68.  --rescore-mode 0 --filter-hits 1 is the reference's own way into mode 1 (rescorediagonal.cpp:95-99, with
// a warning): left to the reference.  The threshold of --filter-hits 1 comes with our own --score-per-col-thr, as for rescorediagonal-local
static int validateRescoreSubst(Call &c) {
    if (c.f.rescoreMode != 1) return unsupported("plass-hip rescorediagonal-subst: --rescore-mode %d is not this module's (1, the substitution score, only)\n", c.f.rescoreMode);
    if (c.f.wrapped || c.f.sortResults > 0) return unsupported("plass-hip rescorediagonal-subst: --wrapped-scoring 1 / --sort-results are not part of the GPU path\n");
    if (c.f.filterHits && !c.f.seen.count("--score-per-col-thr"))
        return unsupported("plass-hip rescorediagonal-subst: --filter-hits 1 needs --score-per-col-thr X (the reference's threshold table is not part of this build)\n");
    return c.pos.size() == 4 && c.pos[0] != c.pos[1] ? unsupported("plass-hip rescorediagonal-subst: separate query and target DBs are not part of the GPU path (linclust uses one DB)\n") : 0;
}
// clust-greedy (our own name: `clust` stays with the reference): clust's greedy modes, Parameters::GREEDY = 2 and GREEDY_MEM = 3, which both run
// greedyIncrementalLowMem (Clustering.cpp:42-47).  The module's default is set cover: a call without --cluster-mode is the reference's.
static int validateClustMode(Call &c) {
    return c.f.clusterMode != 2 && c.f.clusterMode != 3
        ? unsupported("plass-hip %s: --cluster-mode %d is not part of the GPU path (2 and 3, the greedy modes, only)\n", c.m->name, c.f.clusterMode) : 0;
}
static int validateClustResultDb(Call &c) {
    if (c.pos.size() != 3) return 0;
    const int dbtype = probeDbtype(c.pos[1]);     // prefilter DBs (7, 14) and alignment DBs (5)
    return dbtype >= 0 && dbtype != PLASSHIP_DBTYPE_PREFILTER_RES && dbtype != PLASSHIP_DBTYPE_PREFILTER_REV_RES && dbtype != PLASSHIP_DBTYPE_ALIGNMENT_RES
        ? unsupported("plass-hip %s: a result DB of type %d is not part of the GPU path (prefilter and alignment DBs only)\n", c.m->name, dbtype) : 0;
}
static int validateClustGreedy(Call &c) {
    if (const int rc = validateClustMode(c)) return rc;
    return validateClustResultDb(c);
}
// connected component, Parameters::CONNECTED_COMPONENT = 1: --max-iterations is the depth of its breadth-first search and matches ^[1-9]{1}[0-9]*$
// in the reference (Parameters.cpp:91), which ends with "Error in argument" otherwise
static int validateMaxIterations(Call &c) {
    if (c.f.maxIterations >= 1) return 0;
    fprintf(stdout, "Error in argument --max-iterations\n");
    return EXIT_FAILURE;
}
// clust-connected (our own name: `clust` stays with the reference): the one mode this module is; a call without --cluster-mode is the reference's set cover
static int validateClustConnected(Call &c) {
    if (c.f.clusterMode != 1)
        return unsupported("plass-hip clust-connected: --cluster-mode %d is not this module's (1, connected component, only; 2 and 3: clust-greedy)\n", c.f.clusterMode);
    if (const int rc = validateMaxIterations(c)) return rc;
    return validateClustResultDb(c);
}
// the fused drivers run both `clust` calls of linclust.sh:35,82 in the mode they are given: greedy (2, 3) or connected component (1)
static int validateClustModeDriver(Call &c) {
    if (c.f.clusterMode == 1) return validateMaxIterations(c);
    return c.f.clusterMode != 2 && c.f.clusterMode != 3
        ? unsupported("plass-hip %s: --cluster-mode %d is not part of the GPU path (1, connected component, and 2 and 3, the greedy modes, only)\n", c.m->name, c.f.clusterMode) : 0;
}
// linclust-pre: linclust.sh:21-57 from the sequence DB to pre_clust and pref_filter2, one DB as query and target
static int validateLinclustPre(Call &c) {
    if (const int rc = validateClustMode(c)) return rc;
    if (const int rc = validateKmermatcher(c)) return rc;
    return validateRescoreHamming(c);
}
// mergeclusters-greedy (our own name: `mergeclusters` stays with the reference): the reference merges any number of clusterings, linclust passes two
static int validateMergeclusters(Call &c) {
    return c.pos.size() >= 3 && c.pos.size() != 4 ? unsupported("plass-hip mergeclusters-greedy: %zu clusterings are not part of the GPU path (exactly two, as linclust passes them)\n", c.pos.size() - 2) : 0;
}
// linclust-ungapped: the whole of linclust.sh with --alignment-mode 4 on a nucleotide DB, from the sequence DB to the merged clustering.  The workflow
// sets --rescore-mode for its steps itself (0, then 2) and runs the alignment with --filter-hits 1 (workflow/Linclust.cpp:103-127: filterHits is set for step 3
// and stays set), so the threshold has to come with --score-per-col-thr unless --filter-hits 0 is given.  A protein DB has the workflow's extra
// filter step 3 (linclust.sh:59-68), which is not built
static int validateLinclustUngapped(Call &c) {
    if (const int rc = validateClustModeDriver(c)) return rc;
    if (const int rc = validateKmermatcher(c)) return rc;
    if (c.f.seen.count("--rescore-mode") && c.f.rescoreMode != 2) return unsupported("plass-hip linclust-ungapped: --rescore-mode %d is not this driver's (its alignment step is mode 2)\n", c.f.rescoreMode);
    // (the reference's mode 2 ends with "wrapped scoring is only allowed with RESCORE_MODE_HAMMING", and the workflow passes one flag set to both steps)
    if (c.f.wrapped || c.f.sortResults > 0) return unsupported("plass-hip linclust-ungapped: --wrapped-scoring 1 / --sort-results are not part of the GPU path\n");
    if (c.f.filterHits && !c.f.seen.count("--score-per-col-thr"))
        return unsupported("plass-hip linclust-ungapped: the workflow's alignment step runs with --filter-hits 1, which needs --score-per-col-thr X (the reference's threshold table is not part of this build); or give --filter-hits 0\n");
    if (c.pos.size() == 2 && probeDbtype(c.pos[0]) == PLASSHIP_DBTYPE_AMINO_ACIDS)
        return unsupported("plass-hip linclust-ungapped: a protein DB is not part of the GPU path (nucleotide DBs only: the protein workflow has a filter step more, see linclust-ungapped-prot)\n");
    return !c.f.repOut.empty() && existsAlready(c.f.repOut) ? EXIT_FAILURE : 0;
}
// linclust-ungapped-prot: linclust.sh with --alignment-mode 4 and FILTER=1 (amino-acid DBs, Linclust.cpp:95): the mode 1 filter step between the
// subset of the prefilter list and the alignment.  Both rescore steps run with --filter-hits 1 and look their threshold up with the same
// --min-seq-id, -c and --cov-mode (Linclust.cpp:116-127), so one --score-per-col-thr serves both
static int validateLinclustUngappedProt(Call &c) {
    if (const int rc = validateClustModeDriver(c)) return rc;
    if (const int rc = validateKmermatcher(c)) return rc;
    if (c.f.seen.count("--rescore-mode") && c.f.rescoreMode != 2) return unsupported("plass-hip linclust-ungapped-prot: --rescore-mode %d is not this driver's (its alignment step is mode 2)\n", c.f.rescoreMode);
    if (c.f.wrapped || c.f.sortResults > 0) return unsupported("plass-hip linclust-ungapped-prot: --wrapped-scoring 1 / --sort-results are not part of the GPU path\n");
    if (c.f.filterHits && !c.f.seen.count("--score-per-col-thr"))
        return unsupported("plass-hip linclust-ungapped-prot: the workflow's filter and alignment steps run with --filter-hits 1, which needs --score-per-col-thr X (the reference's threshold table is not part of this build); or give --filter-hits 0\n");
    if (c.pos.size() == 2 && probeDbtype(c.pos[0]) == PLASSHIP_DBTYPE_NUCLEOTIDES)
        return unsupported("plass-hip linclust-ungapped-prot: a nucleotide DB is not this driver's (the nucleotide workflow has no filter step: linclust-ungapped)\n");
    return !c.f.repOut.empty() && existsAlready(c.f.repOut) ? EXIT_FAILURE : 0;
}
// Requests that are valid for the reference and lie outside the GPU path are all refused in validate(), before the dry-run exit and before anything
// is read or written (data/nuclassemble.sh:41,145 calls `concatdbs ... --preserve-keys` whenever circular contigs exist; with exit
// code 1 the wrapper ended the workflow instead of handing the call to the reference, and the dry run reported it as accepted)
static int validateConcatdbs(Call &c) {
    if (c.f.takeLarger) return unsupported("plass-hip concatdbs: --take-larger-entry is not part of the GPU path\n");
    if (c.pos.size() != 3) return 0;
    const int dbtype = probeDbtype(c.pos[0]);     // sequence DBs, or the header DBs of ORF DBs (dbtype 12: data/assemble.sh:75)
    if (dbtype >= 0 && dbtype != PLASSHIP_DBTYPE_AMINO_ACIDS && dbtype != PLASSHIP_DBTYPE_NUCLEOTIDES && dbtype != 12)
        return unsupported("plass-hip concatdbs: database type %d is not part of the GPU path (sequence DBs and ORF header DBs only)\n", dbtype);
    return dbtype == 12 && c.f.preserveKeys ? unsupported("plass-hip concatdbs: --preserve-keys on a header DB is not part of the GPU path\n") : 0;
}
static int validateProteinaln2nucl(Call &c) {
    const std::vector<std::string> &pos = c.pos;
    if (pos.size() != 6) return 0;
    if ((pos[0] == pos[1]) != (pos[2] == pos[3])) { fprintf(stdout, "Either query database == target database for nucleotide and amino acid or != for both\n"); return EXIT_FAILURE; }
    return pos[0] != pos[1] ? unsupported("plass-hip proteinaln2nucl: separate query and target DBs are not part of the GPU path (the assembly workflows use one DB)\n") : 0;
}
static int validateCreatedbReads(Call &c) {
    const Flags &f = c.f;
    if (c.pos.size() < 2) { fprintf(stdout, "%s\n", c.m->usage); return EXIT_FAILURE; }
    if (f.createdbMode != 0) return unsupported("plass-hip createdb-reads: --createdb-mode %d (soft links) is left to the reference\n", f.createdbMode);
    if (f.writeLookup != 1) return unsupported("plass-hip createdb-reads: --write-lookup %d is left to the reference\n", f.writeLookup);
    if (f.dbtypeArg < 0 || f.dbtypeArg > 2) { fprintf(stdout, "Error in argument --dbtype\n"); return EXIT_FAILURE; }
    if (f.dbtypeArg == 1) return unsupported("plass-hip createdb-reads: --dbtype 1 (amino acids) is not an input of the assembly workflows; left to the reference\n");
    if (f.idOffset > 0xFFFFFFFEull) { fprintf(stdout, "Error in argument --id-offset\n"); return EXIT_FAILURE; }
    return takeReadFiles(c, 1);
}
static int validateMergereads(Call &c) {
    if (c.pos.size() < 3 || (c.pos.size() - 1) % 2) { fprintf(stdout, "%s\n", c.m->usage); return EXIT_FAILURE; }
    return takeReadFiles(c, 1);
}
static int validateChain(Call &c) {
    const Flags &f = c.f; const std::vector<std::string> &pos = c.pos; const char *mod = c.m->name; const size_t nOut = nChainOut(c);
    if (c.m->id & ORF_CHAINS) if (const int rc = validateGencode(c)) return rc;      // --translation-table: the workflows hand it to extractorfs and translatenucs
    if (f.singleEnd) {      // every positional before the output(s) is an unpaired read file (data/assemble.sh:27-38: createdb in place of mergereads)
        if (pos.size() < nOut + 1) { fprintf(stdout, "%s: --single-end 1 needs at least one read file before the output\n", mod); return EXIT_FAILURE; }
    } else if (pos.size() > nOut + 1 && (pos.size() - nOut) % 2) { fprintf(stdout, "%s: one DB or pairs of FASTQ files before the output\n", mod); return EXIT_FAILURE; }
    if (f.singleEnd || pos.size() > nOut + 1) if (const int rc = takeReadFiles(c, nOut)) return rc;
    // --fasta-out: the workflows' tail on the device (data/assemble.sh:159-201, nuclassemble.sh:138-207).  With --filter-proteins 1 (plass
    // assemble's default) the tail selects from filternoncoding's output, a network with the reference's weights: not on this path.
    auto refusedOutput = [&](const std::string &o) {        // what every output of a tail is checked for (--contig-output-mode: the nucleotide workflows' flag)
        if (f.contigOutputMode != 0 && f.contigOutputMode != 1) { fprintf(stdout, "--contig-output-mode must be 0 or 1\n"); return true; }
        return existsAlready(o);
    };
    if (!f.fastaOut.empty()) {
        if (c.m->id == ASSEMBLE_CHAIN && f.filterProteins != 0)
            return unsupported("plass-hip assemble-chain: --fasta-out selects from filternoncoding's output with --filter-proteins 1; filternoncoding is outside the GPU path (pass --filter-proteins 0)\n");
        if (refusedOutput(f.fastaOut)) return EXIT_FAILURE;
    }
    // --db-mode 1 --db-out DB (nuclassemble-chain) and --nuclassembly-out DB (guidedassemble-chain): the same tail ending in createsubdb's DB
    // instead of the FASTA file (nuclassemble.sh:200-207; the guided workflow runs its nuclassemble with --db-mode 1, GuidedNuclassembler.cpp:173)
    if (f.dbMode || !f.dbOut.empty()) {
        if (f.dbMode && !f.fastaOut.empty()) { fprintf(stdout, "nuclassemble-chain: --db-mode 1 writes a DB (--db-out), not a FASTA file: --fasta-out cannot be combined with it\n"); return EXIT_FAILURE; }
        if (!f.dbMode || f.dbOut.empty()) { fprintf(stdout, "nuclassemble-chain: --db-mode 1 and --db-out DB go together\n"); return EXIT_FAILURE; }
    }
    for (const std::string *o : {&f.dbOut, &f.nuclAssemblyOut}) if (!o->empty() && refusedOutput(*o)) return EXIT_FAILURE;
    if (!f.nuclAssemblyOut.empty() && f.numIterationsNucl < 1) { fprintf(stdout, "--num-iterations must be at least 1 (nucl)\n"); return EXIT_FAILURE; }
    // --resume 1 (assemble-chain, nuclassemble-chain): go on behind the highest complete DIR/assembly_<j> of an earlier run with the same
    // --write-intermediate DIR.  What cannot be right is refused here, before anything is read: a continuation with other parameters or
    // another input than DIR/chain.manifest records would be a chimera of two runs.
    if (!f.resume) return 0;
    // (guided: --write-intermediate keeps assembly_nucl_<i> only; the protein twins guidedassembleresults extends next to it, guidedassembleresult.cpp:340-365, are not stored)
    if (c.m->id == GUIDEDASSEMBLE_CHAIN) { fprintf(stdout, "guidedassemble-chain: --resume is not supported: --write-intermediate stores the nucleotide assembly without its protein twins, which is not enough to restart\n"); return EXIT_FAILURE; }
    if (f.writeIntermediate.empty()) { fprintf(stdout, "%s: --resume 1 needs --write-intermediate DIR (the resume points are DIR/assembly_<i>)\n", mod); return EXIT_FAILURE; }
    std::vector<std::string> inputs = c.readFiles;
    if (inputs.empty() && !pos.empty()) for (const char *sfx : {"", ".index", ".dbtype"}) inputs.push_back(pos[0] + sfx);
    c.manifest = chainManifest(mod, f, inputs);
    c.resumeFrom = resumePoint(f.writeIntermediate, "assembly_", f.numIterations);
    if (c.resumeFrom < 0) return 0;
    const std::string mp = f.writeIntermediate + "/chain.manifest";
    if (!isFile(mp)) {
        fprintf(stdout, "%s: --resume 1: %s/assembly_%d.done exists but %s does not: what the stored DBs were computed with is unknown (delete the .done files to start over)\n",
                mod, f.writeIntermediate.c_str(), c.resumeFrom, mp.c_str());
        return EXIT_FAILURE;
    }
    std::string inFile; const std::string key = manifestDiffers(mp, c.manifest, inFile);
    if (key.empty()) return 0;
    std::string now; for (const auto &kv : c.manifest) if (kv.first == key) now = kv.second;
    fprintf(stdout, "%s: --resume 1: %s differs from the run that wrote %s/assembly_%d (%s: %s, this run: %s); delete the .done files to start over\n",
            mod, key.c_str(), f.writeIntermediate.c_str(), c.resumeFrom, mp.c_str(), inFile.c_str(), now.c_str());
    return EXIT_FAILURE;
}

// ---- the modules' bodies: read, call, print, write.  Every handle is released when its body returns, before main()'s epilogue. ----
static int runKmermatcher(Call &c) {
    plasship_ctx *ctx = c.ctx; SeqDb db(ctx); Cands cands(ctx);
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail("kmermatcher");
    const plasship_kmermatch_params p = kmermatchParams(c.f, dbtypeOf(db) == PLASSHIP_DBTYPE_NUCLEOTIDES ? c.f.scaleNucl : c.f.scaleAA); plasship_kmermatch_stats st = {};
    if (K(plasship_kmermatch(ctx, db, &p, cands.out(), &st))) return fail("kmermatcher");
    fprintf(stdout, "k-mer records: %llu grouped: %llu candidates: %llu | kernels ms: extract %.3f partition %.3f group %.3f sort %.3f reduce %.3f\n",
            (unsigned long long) st.n_kmer_records, (unsigned long long) st.n_grouped, (unsigned long long) st.n_candidates,
            st.ms_extract, st.ms_sort1, st.ms_group, st.ms_sort2, st.ms_reduce);
    return KW(plasship_cands_write(ctx, cands, db, c.pos[1].c_str())) ? fail("kmermatcher") : EXIT_SUCCESS;
}
static int runRescorediagonal(Call &c) {
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    SeqDb q(ctx), tOwn(ctx); Cands cands(ctx); Alns al(ctx);
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), q.out()))) return fail("rescorediagonal");
    if (pos[1] != pos[0] && K(plasship_seqdb_read(ctx, pos[1].c_str(), tOwn.out()))) return fail("rescorediagonal");
    const plasship_seqdb *t = pos[1] == pos[0] ? q.p : tOwn.p;       // one handle for query == target: the plass case (sameQTDB)
    if (K(plasship_cands_read(ctx, q, t, pos[2].c_str(), cands.out()))) return fail("rescorediagonal");
    const plasship_rescore_params p = rescoreParams(c.f); plasship_rescore_stats st = {};
    if (K(plasship_rescore(ctx, q, t, cands, &p, al.out(), &st))) return fail("rescorediagonal");
    fprintf(stdout, "scored: %llu accepted: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_scored, (unsigned long long) st.n_accepted, st.ms_kernel);
    return KW(plasship_alns_write(ctx, al, pos[3].c_str())) ? fail("rescorediagonal") : EXIT_SUCCESS;
}
static int runRescoreHamming(Call &c) {           // (query and target are one DB: validateRescoreHamming)
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos; const Flags &f = c.f;
    SeqDb db(ctx); Cands cands(ctx), kept(ctx);
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), db.out())) || K(plasship_cands_read(ctx, db, db, pos[2].c_str(), cands.out()))) return fail("rescorediagonal-hamming");
    const plasship_hamming_params p = hammingParams(f); plasship_rescore_stats st = {};
    if (K(plasship_rescore_hamming(ctx, db, db, cands, &p, kept.out(), &st))) {
        // (wrapped scoring on a DB that is not nucleotides is an error of the call, in the reference as well: not a case for the reference binary)
        return fail("rescorediagonal-hamming");
    }
    fprintf(stdout, "scored: %llu kept: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_scored, (unsigned long long) st.n_accepted, st.ms_kernel);
    return KW(plasship_cands_write(ctx, kept, db, pos[3].c_str())) ? fail("rescorediagonal-hamming") : EXIT_SUCCESS;
}
static int runRescoreLocal(Call &c) {             // (query and target are one DB: validateRescoreLocal)
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    SeqDb db(ctx); Cands cands(ctx); Alns al(ctx);
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), db.out())) || K(plasship_cands_read(ctx, db, db, pos[2].c_str(), cands.out()))) return fail("rescorediagonal-local");
    const plasship_local_params p = localParams(c.f); plasship_rescore_stats st = {};
    if (K(plasship_rescore_local(ctx, db, cands, &p, al.out(), &st))) return fail("rescorediagonal-local");
    fprintf(stdout, "scored: %llu kept: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_scored, (unsigned long long) st.n_accepted, st.ms_kernel);
    return KW(plasship_alns_write(ctx, al, pos[3].c_str())) ? fail("rescorediagonal-local") : EXIT_SUCCESS;
}
static int runRescoreSubst(Call &c) {             // (query and target are one DB: validateRescoreSubst)
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    SeqDb db(ctx); Cands cands(ctx), kept(ctx);
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), db.out())) || K(plasship_cands_read(ctx, db, db, pos[2].c_str(), cands.out()))) return fail("rescorediagonal-subst");
    const plasship_subst_params p = substParams(c.f); plasship_rescore_stats st = {};
    if (K(plasship_rescore_subst(ctx, db, cands, &p, kept.out(), &st))) return fail("rescorediagonal-subst");
    fprintf(stdout, "scored: %llu kept: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_scored, (unsigned long long) st.n_accepted, st.ms_kernel);
    return KW(plasship_cands_write(ctx, kept, db, pos[3].c_str())) ? fail("rescorediagonal-subst") : EXIT_SUCCESS;
}
// DBReader::softlinkDb(seqDB, outDB, SEQUENCE_ANCILLARY) (result2repseq.cpp:54, DBReader.cpp:1089-1154): absolute soft links to the sequence DB's header,
// lookup, source and taxonomy files where those exist
static int linkAncillary(const std::string &seqDb, const std::string &outDb) {
    for (const char *sfx : {"_h", "_h.index", "_h.dbtype", ".lookup", ".source", "_mapping", "_names.dmp", "_nodes.dmp", "_merged.dmp", "_taxonomy"}) {
        const std::string file = seqDb + sfx, link = outDb + sfx;
        struct stat st;
        if (stat(file.c_str(), &st) != 0) continue;
        char *t = realpath(file.c_str(), nullptr);
        if (!t) { fprintf(stdout, "Could not get realpath of %s!\n", file.c_str()); return EXIT_FAILURE; }
        if (lstat(link.c_str(), &st) == 0) unlink(link.c_str());
        const bool ok = symlink(t, link.c_str()) == 0;
        free(t);
        if (!ok) { fprintf(stdout, "Could not create symlink of %s!\n", file.c_str()); return EXIT_FAILURE; }
    }
    return 0;
}
// every entry of a cluster DB on disk starts with its own key (what Clustering::writeData and mergeclusters write; result2repseq takes the FIRST key,
// plasship_clusters_repseqs the entry's) and none is empty (the reference writes no sequence for one): 1, 0 if not, -1 if the files cannot be read
static int clusterListsStartWithOwnKey(const std::string &clu) {
    FILE *fi = fopen((clu + ".index").c_str(), "rb"), *fd = fopen(clu.c_str(), "rb");
    int ok = fi && fd ? 1 : -1;
    unsigned long long key, off, len;
    while (ok == 1 && fscanf(fi, "%llu %llu %llu", &key, &off, &len) == 3) {
        char buf[32] = {0};
        if (len <= 1 || fseeko(fd, (off_t) off, SEEK_SET) != 0 || fread(buf, 1, std::min<size_t>(sizeof(buf) - 1, (size_t) len), fd) == 0) { ok = 0; break; }
        char *end = nullptr; const unsigned long long first = strtoull(buf, &end, 10);
        if (end == buf || first != key) ok = 0;
    }
    if (fi) fclose(fi);
    if (fd) fclose(fd);
    return ok;
}
static int runClustRepseq(Call &c) {              // result2repseq: <seqDB> <cluDB> <outDB>
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    SeqDb db(ctx), rep(ctx); Clusters cl(ctx);
    if (clusterListsStartWithOwnKey(pos[1]) == 0) return unsupported("plass-hip clust-repseq: %s has an empty entry or a list that does not start with its own key\n", pos[1].c_str());
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), db.out()))) return fail("clust-repseq");
    // (a cluster DB the reader cannot take — a key listed twice, a list that does not start with its own key — is left to the reference: nothing has been written)
    if (K(plasship_clusters_read(ctx, db, pos[1].c_str(), cl.out())))
        return g_lastRc == PLASSHIP_ERR_ARG ? unsupported("plass-hip clust-repseq: %s\n", plasship_last_error()) : fail("clust-repseq");
    if (K(plasship_clusters_repseqs(ctx, cl, db, rep.out()))) return fail("clust-repseq");
    size_t n = 0; plasship_seqdb_info(rep, &n, nullptr, nullptr, nullptr, nullptr);
    fprintf(stdout, "representatives: %zu\n", n);
    if (KW(plasship_seqdb_write(ctx, rep, pos[2].c_str()))) return fail("clust-repseq");
    return linkAncillary(pos[0], pos[2]);
}
static long indexLines(const std::string &db) {       // entries of a DB on disk; -1: no index
    FILE *fi = fopen((db + ".index").c_str(), "rb"); if (!fi) return -1;
    long n = 0; char buf[65536]; size_t got;
    while ((got = fread(buf, 1, sizeof(buf), fi)) > 0) for (size_t i = 0; i < got; i++) n += buf[i] == '\n';
    fclose(fi);
    return n;
}
static void printClustStats(const plasship_clust_stats &st) {
    fprintf(stdout, "sequences: %llu edges: %llu clusters: %llu promoted: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_sequences, (unsigned long long) st.n_edges,
            (unsigned long long) st.n_clusters, (unsigned long long) st.n_promoted, st.ms_kernel);
}
static void printCcStats(const plasship_cc_stats &st) {
    fprintf(stdout, "sequences: %llu edges: %llu clusters: %llu missing links: %llu | hook rounds: %u bfs levels: %u | kernel ms: %.3f\n", (unsigned long long) st.n_sequences,
            (unsigned long long) st.n_edges, (unsigned long long) st.n_clusters, (unsigned long long) st.n_missing_links, st.n_hook_rounds, st.n_bfs_levels, st.ms_kernel);
}
static int runClust(Call &c) {                    // clust-greedy and clust-connected: <seqDB> <resultDB> <cluDB>
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos; const char *name = c.m->name; const bool connected = c.m->id == CLUST_CONNECTED;
    SeqDb db(ctx); Cands cands(ctx); Alns al(ctx); Clusters cl(ctx); plasship_clust_stats st = {}; plasship_cc_stats cs = {};
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), db.out()))) return fail(name);
    size_t n = 0; plasship_seqdb_info(db, &n, nullptr, nullptr, nullptr, nullptr);
    if (indexLines(pos[1]) != (long) n) { fprintf(stdout, "Sequence db size != result db size\n"); return EXIT_FAILURE; }      // ClusteringAlgorithms.cpp:20-23
    if (probeDbtype(pos[1]) == PLASSHIP_DBTYPE_ALIGNMENT_RES) {
        // (lines plasship_alns_read cannot take — fewer than ten columns — are left to the reference: nothing has been written)
        if (K(plasship_alns_read(ctx, db, pos[1].c_str(), al.out())))
            return g_lastRc == PLASSHIP_ERR_ARG ? unsupported("plass-hip %s: %s\n", name, plasship_last_error()) : fail(name);
        if (K(connected ? plasship_clust_connected_alns(ctx, db, al, c.f.maxIterations, cl.out(), &cs) : plasship_clust_greedy_alns(ctx, db, al, cl.out(), &st))) return fail(name);
    } else {
        if (K(plasship_cands_read(ctx, db, db, pos[1].c_str(), cands.out())) ||
            K(connected ? plasship_clust_connected_cands(ctx, db, cands, c.f.maxIterations, cl.out(), &cs) : plasship_clust_greedy_cands(ctx, db, cands, cl.out(), &st))) return fail(name);
    }
    if (connected) printCcStats(cs); else printClustStats(st);
    return KW(plasship_clusters_write(ctx, cl, db, pos[2].c_str())) ? fail(name) : EXIT_SUCCESS;
}
static int runLinclustPre(Call &c) {              // kmermatcher -> rescorediagonal (Hamming) -> clust -> createsubdb + filterdb of pref, on handles
    plasship_ctx *ctx = c.ctx; const Flags &f = c.f;
    SeqDb db(ctx); Cands pref(ctx), rescored(ctx), filtered(ctx); Clusters cl(ctx);
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail("linclust-pre");
    const plasship_kmermatch_params kp = kmermatchParams(f, dbtypeOf(db) == PLASSHIP_DBTYPE_NUCLEOTIDES ? f.scaleNucl : f.scaleAA); plasship_kmermatch_stats ks = {};
    const plasship_hamming_params hp = hammingParams(f); plasship_rescore_stats rs = {}; plasship_clust_stats st = {};
    if (K(plasship_kmermatch(ctx, db, &kp, pref.out(), &ks)) || K(plasship_rescore_hamming(ctx, db, db, pref, &hp, rescored.out(), &rs)) ||
        K(plasship_clust_greedy_cands(ctx, db, rescored, cl.out(), &st)) || K(plasship_cands_filter(ctx, pref, cl, filtered.out()))) return fail("linclust-pre");
    fprintf(stdout, "candidates: %llu scored: %llu kept: %llu | kernel ms: hamming %.3f\n", (unsigned long long) ks.n_candidates, (unsigned long long) rs.n_scored,
            (unsigned long long) rs.n_accepted, rs.ms_kernel);
    printClustStats(st);
    return KW(plasship_clusters_write(ctx, cl, db, c.pos[1].c_str())) || KW(plasship_cands_write(ctx, filtered, db, c.pos[2].c_str())) ? fail("linclust-pre") : EXIT_SUCCESS;
}
static int runMergeclusters(Call &c) {            // (exactly two clusterings: validateMergeclusters)
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    SeqDb db(ctx); Clusters first(ctx), second(ctx); Merged mg(ctx);
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), db.out()))) return fail("mergeclusters-greedy");
    // (a clustering the reader cannot take — a key listed twice, a representative listed under another one — is left to the reference: nothing has been written)
    if (K(plasship_clusters_read(ctx, db, pos[2].c_str(), first.out())) || K(plasship_clusters_read(ctx, db, pos[3].c_str(), second.out())) ||
        K(plasship_clusters_merge(ctx, db, first, second, mg.out())))
        return g_lastRc == PLASSHIP_ERR_ARG ? unsupported("plass-hip mergeclusters-greedy: %s\n", plasship_last_error()) : fail("mergeclusters-greedy");
    uint64_t n = 0, nC = 0; plasship_merged_count(mg, &n, &nC);
    fprintf(stdout, "sequences: %llu clusters: %llu\n", (unsigned long long) n, (unsigned long long) nC);
    return KW(plasship_merged_write(ctx, mg, db, pos[1].c_str())) ? fail("mergeclusters-greedy") : EXIT_SUCCESS;
}
// linclust-pre's chain, then (linclust-ungapped-prot: the mode 1 filter on the representatives, then) mode 2 on the representatives -> clust -> mergeclusters, on handles
static int runLinclustUngapped(Call &c) {
    plasship_ctx *ctx = c.ctx; const Flags &f = c.f; const char *name = c.m->name; const bool prot = c.m->id == LINCLUST_UNGAPPED_PROT;
    SeqDb db(ctx); Cands pref(ctx), rescored(ctx), filtered(ctx); Clusters pre(ctx), cl(ctx); Alns al(ctx); Merged mg(ctx);
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail(name);
    if (!prot && dbtypeOf(db) != PLASSHIP_DBTYPE_NUCLEOTIDES) return unsupported("plass-hip linclust-ungapped: nucleotide DBs only\n");
    if (prot && dbtypeOf(db) != PLASSHIP_DBTYPE_AMINO_ACIDS) return unsupported("plass-hip linclust-ungapped-prot: amino-acid DBs only\n");
    const plasship_kmermatch_params kp = kmermatchParams(f, prot ? f.scaleAA : f.scaleNucl); plasship_kmermatch_stats ks = {};
    plasship_hamming_params hp = hammingParams(f);      // Linclust.cpp:106-111: the Hamming step never goes below 0.5 in seq. id. and coverage
    hp.seq_id_thr = std::max(0.5f, f.seqIdThr); hp.cov_thr = std::max(0.5f, f.covThr);
    const plasship_local_params lp = localParams(f); const plasship_subst_params sp = substParams(f);
    plasship_rescore_stats rs = {}, fs = {}, ls = {}; plasship_clust_stats st = {}, st2 = {}; plasship_cc_stats cs = {}, cs2 = {};
    const bool connected = f.clusterMode == 1;    // both `clust` calls of linclust.sh:35,82 run in the workflow's one mode
    if (K(plasship_kmermatch(ctx, db, &kp, pref.out(), &ks)) || K(plasship_rescore_hamming(ctx, db, db, pref, &hp, rescored.out(), &rs)) ||
        K(connected ? plasship_clust_connected_cands(ctx, db, rescored, f.maxIterations, pre.out(), &cs) : plasship_clust_greedy_cands(ctx, db, rescored, pre.out(), &st)) ||
        K(plasship_cands_filter(ctx, pref, pre, filtered.out()))) return fail(name);
    if (prot) {                                   // linclust.sh:59-68: pref_filter2 -> pref_rescore2
        Cands passed(ctx);
        if (K(plasship_rescore_subst_subset(ctx, db, filtered, pre, &sp, passed.out(), &fs))) return fail(name);
        filtered = std::move(passed);
    }
    if (K(plasship_rescore_local_subset(ctx, db, filtered, pre, &lp, al.out(), &ls)) ||
        K(connected ? plasship_clust_connected_alns(ctx, db, al, f.maxIterations, cl.out(), &cs2) : plasship_clust_greedy_alns(ctx, db, al, cl.out(), &st2)) ||
        K(plasship_clusters_merge(ctx, db, pre, cl, mg.out()))) return fail(name);
    fprintf(stdout, "candidates: %llu scored: %llu kept: %llu | aligned: %llu kept: %llu | kernel ms: hamming %.3f local %.3f\n", (unsigned long long) ks.n_candidates,
            (unsigned long long) rs.n_scored, (unsigned long long) rs.n_accepted, (unsigned long long) ls.n_scored, (unsigned long long) ls.n_accepted, rs.ms_kernel, ls.ms_kernel);
    if (prot) fprintf(stdout, "filtered: %llu kept: %llu | kernel ms: subst %.3f\n", (unsigned long long) fs.n_scored, (unsigned long long) fs.n_accepted, fs.ms_kernel);
    if (connected) { printCcStats(cs); printCcStats(cs2); } else printClustStats(st);
    uint64_t n = 0, nC = 0; plasship_merged_count(mg, &n, &nC);
    fprintf(stdout, "sequences: %llu clusters: %llu\n", (unsigned long long) n, (unsigned long long) nC);
    if (KW(plasship_merged_write(ctx, mg, db, c.pos[1].c_str()))) return fail(name);
    if (!f.repOut.empty()) {                      // result2repseq of the merged clustering, with its soft links (guidedNuclAssemble.sh:182-186)
        SeqDb rep(ctx);
        if (K(plasship_merged_repseqs(ctx, mg, db, rep.out())) || KW(plasship_seqdb_write(ctx, rep, f.repOut.c_str()))) return fail(name);
        if (const int rc = linkAncillary(c.pos[0], f.repOut)) return rc;
    }
    return EXIT_SUCCESS;
}
static int runAssembleresults(Call &c) {          // assembleresults and nuclassembleresults
    plasship_ctx *ctx = c.ctx; SeqDb db(ctx); Alns al(ctx); SeqDb o(ctx);
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail("assembleresults");
    // the library picks the variant from the DB type (protein -> assembleresults, nucleotide -> nuclassembleresults);
    // the module name has to agree, the reference's assembleresults on nucleotides uses another comparator
    const bool nucl = c.m->id == NUCLASSEMBLERESULTS;
    if (nucl != (dbtypeOf(db) == PLASSHIP_DBTYPE_NUCLEOTIDES)) { fprintf(stdout, "plass-hip: %s needs a %s sequence DB\n", c.m->name, nucl ? "nucleotide" : "protein"); return EXIT_FAILURE; }
    if (K(plasship_alns_read(ctx, db, c.pos[1].c_str(), al.out()))) return fail("assembleresults");
    const plasship_assemble_params p = assembleParams(c.f); plasship_assemble_stats st = {};
    if (K(plasship_assemble(ctx, db, al, &p, o.out(), &st))) return fail("assembleresults");
    fprintf(stdout, "extended: %llu rescored: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_extended, (unsigned long long) st.n_rescored, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, o, c.pos[2].c_str())) ? fail("assembleresults") : EXIT_SUCCESS;
}
static int runGuidedassembleresults(Call &c) {
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    SeqDb nu(ctx), aa(ctx); Alns al(ctx); SeqDb oa(ctx), on(ctx);
    if (K(plasship_seqdb_read(ctx, pos[0].c_str(), nu.out())) || K(plasship_seqdb_read(ctx, pos[1].c_str(), aa.out()))) return fail("guidedassembleresults");
    if (K(plasship_alns_read(ctx, nu, pos[2].c_str(), al.out()))) return fail("guidedassembleresults");
    const plasship_assemble_params p = assembleParams(c.f); plasship_assemble_stats st = {};
    if (K(plasship_guided_assemble(ctx, nu, aa, al, &p, on.out(), oa.out(), &st))) return fail("guidedassembleresults");
    fprintf(stdout, "extended: %llu rescored: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_extended, (unsigned long long) st.n_rescored, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, on, pos[3].c_str())) || KW(plasship_seqdb_write(ctx, oa, pos[4].c_str())) ? fail("guidedassembleresults") : EXIT_SUCCESS;
}
static int runProteinaln2nucl(Call &c) {          // (query and target are one DB: validateProteinaln2nucl)
    plasship_ctx *ctx = c.ctx; SeqDb nu(ctx), aa(ctx); Alns al(ctx), o(ctx);
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), nu.out())) || K(plasship_seqdb_read(ctx, c.pos[2].c_str(), aa.out()))) return fail("proteinaln2nucl");
    if (K(plasship_alns_read(ctx, aa, c.pos[4].c_str(), al.out()))) return fail("proteinaln2nucl");
    const plasship_aln2nucl_params p = aln2nuclParams(c.f); plasship_aln2nucl_stats st = {};
    if (K(plasship_aln2nucl(ctx, nu, nu, aa, aa, al, &p, o.out(), &st))) return fail("proteinaln2nucl");
    fprintf(stdout, "alignments: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_alignments, st.ms_kernel);
    return KW(plasship_alns_write(ctx, o, c.pos[5].c_str())) ? fail("proteinaln2nucl") : EXIT_SUCCESS;
}
static int runFindassemblystart(Call &c) {
    plasship_ctx *ctx = c.ctx; SeqDb db(ctx); Alns al(ctx); SeqDb o(ctx); plasship_findstart_stats st = {};
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail("findassemblystart");
    if (K(plasship_alns_read(ctx, db, c.pos[1].c_str(), al.out()))) return fail("findassemblystart");
    if (K(plasship_find_assembly_start(ctx, db, al, o.out(), &st))) return fail("findassemblystart");
    fprintf(stdout, "alignments: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_alignments, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, o, c.pos[2].c_str())) ? fail("findassemblystart") : EXIT_SUCCESS;
}
static int runCyclecheck(Call &c) {
    plasship_ctx *ctx = c.ctx; SeqDb db(ctx), o(ctx);
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail("cyclecheck");
    const plasship_cyclecheck_params p = cyclecheckParams(c.f); plasship_cyclecheck_stats st = {};
    if (K(plasship_cyclecheck(ctx, db, &p, o.out(), nullptr, &st))) return fail("cyclecheck");
    fprintf(stdout, "circular: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_cyclic, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, o, c.pos[1].c_str())) ? fail("cyclecheck") : EXIT_SUCCESS;
}
// the genetic code of a call: the standard one with ATG goes through the entry points that know nothing else, any other through libplasship_gencode.so
static bool standardCode(int table, int allStarts) { return table == 1 && !allStarts; }
static int extractOrfs(plasship_ctx *ctx, const plasship_seqdb *reads, const plasship_orf_params &p, plasship_seqdb **orfs, plasship_orfhdr **hdr, plasship_orf_stats *st) {
    return standardCode(p.translation_table, p.use_all_table_starts) ? plasship_extract_orfs(ctx, reads, &p, orfs, hdr, st) : plasship_extract_orfs_gc(ctx, reads, &p, orfs, hdr, st);
}
static int translateNucs(plasship_ctx *ctx, const plasship_seqdb *orfs, const plasship_orfhdr *hdr, const plasship_translate_params &p, plasship_seqdb **aa, plasship_orf_stats *st) {
    return p.translation_table == 1 ? plasship_translate_nucs(ctx, orfs, hdr, &p, aa, st) : plasship_translate_nucs_gc(ctx, orfs, hdr, &p, aa, st);
}
static int runExtractorfs(Call &c) {              // writes <out> and <out>_h like the reference (extractorfs.cpp:28-32); extractorfs-gencode: with any genetic code
    plasship_ctx *ctx = c.ctx; SeqDb db(ctx), o(ctx); OrfHdr h(ctx); const char *name = c.m->name;
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail(name);
    const plasship_orf_params p = orfParams(c.f); plasship_orf_stats st = {};
    if (K(c.m->id == EXTRACTORFS_GENCODE ? plasship_extract_orfs_gc(ctx, db, &p, o.out(), h.out(), &st) : plasship_extract_orfs(ctx, db, &p, o.out(), h.out(), &st))) return fail(name);
    fprintf(stdout, "orfs: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_out, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, o, c.pos[1].c_str())) || KW(plasship_orfhdr_write(ctx, h, (c.pos[1] + "_h").c_str())) ? fail(name) : EXIT_SUCCESS;
}
static int runTranslatenucs(Call &c) {
    plasship_ctx *ctx = c.ctx; SeqDb db(ctx), o(ctx); OrfHdr h(ctx); const char *name = c.m->name;
    if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), db.out()))) return fail(name);
    if (c.f.addOrfStop && K(plasship_orfhdr_read(ctx, (c.pos[0] + "_h").c_str(), h.out()))) return fail(name);      // translatenucs.cpp:29-34
    plasship_translate_params p; p.translation_table = c.f.translationTable; p.add_orf_stop = c.f.addOrfStop; p.max_seq_len = c.f.maxSeqLen; plasship_orf_stats st = {};
    if (K(c.m->id == TRANSLATENUCS_GENCODE ? plasship_translate_nucs_gc(ctx, db, h, &p, o.out(), &st) : plasship_translate_nucs(ctx, db, h, &p, o.out(), &st))) return fail(name);
    fprintf(stdout, "translated: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_out, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, o, c.pos[1].c_str())) ? fail(name) : EXIT_SUCCESS;
}
static int runConcatdbs(Call &c) {                // sequence DBs, or the header DBs of ORF DBs (dbtype 12: data/assemble.sh:75); other types: validateConcatdbs
    plasship_ctx *ctx = c.ctx; const std::vector<std::string> &pos = c.pos;
    const int dbtype = probeDbtype(pos[0]);
    if (dbtype == PLASSHIP_DBTYPE_AMINO_ACIDS || dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES) {
        SeqDb a(ctx), b(ctx), o(ctx);
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), a.out())) || K(plasship_seqdb_read(ctx, pos[1].c_str(), b.out()))) return fail("concatdbs");
        if (K(plasship_seqdb_concat_keys(ctx, a, b, c.f.preserveKeys, o.out()))) return fail("concatdbs");
        if (KW(plasship_seqdb_write(ctx, o, pos[2].c_str()))) return fail("concatdbs");
    } else if (dbtype == 12) {
        OrfHdr a(ctx), b(ctx), o(ctx);
        if (K(plasship_orfhdr_read(ctx, pos[0].c_str(), a.out())) || K(plasship_orfhdr_read(ctx, pos[1].c_str(), b.out()))) return fail("concatdbs");
        if (K(plasship_orfhdr_concat(ctx, a, b, o.out()))) return fail("concatdbs");
        if (KW(plasship_orfhdr_write(ctx, o, pos[2].c_str()))) return fail("concatdbs");
    } else { fprintf(stdout, "plass-hip concatdbs: cannot read the database type of %s\n", pos[0].c_str()); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}
static int runCreatedbReads(Call &c) {            // writes <out>, <out>_h, <out>.lookup and <out>.source like the reference's createdb (createdb.cpp:84,92-95,291-329)
    const std::vector<const char *> files = cstrs(c.readFiles);
    plasship_createdb_params cp; cp.shuffle = c.f.shuffle; cp.id_offset = (uint32_t) c.f.idOffset; cp.dbtype = c.f.dbtypeArg; plasship_createdb_stats st = {};
    if (KW(plasship_createdb_write(c.ctx, files.data(), files.size(), &cp, c.pos.back().c_str(), nullptr, &st))) return fail("createdb-reads");
    fprintf(stdout, "entries: %llu lines: %llu chunks: %llu | read %.3f s upload %.3f s kernels %.3f ms (write %.3f ms) total %.3f s\n", (unsigned long long) st.entries,
            (unsigned long long) st.lines, (unsigned long long) st.chunks, st.ms_read * 1e-3, st.ms_upload * 1e-3, st.ms_kernel, st.ms_write_kernel, st.ms_total * 1e-3);
    return EXIT_SUCCESS;
}
static int runMergereads(Call &c) {               // writes <out> and <out>_h like the reference (mergereads.cpp:28-31)
    plasship_ctx *ctx = c.ctx; const std::vector<const char *> files = cstrs(c.readFiles);
    SeqDb r(ctx), h(ctx); plasship_merge_stats st = {};
    if (K(plasship_mergereads(ctx, files.data(), files.size(), nullptr, r.out(), h.out(), &st))) return fail("mergereads");
    fprintf(stdout, "pairs: %llu combined: %llu not combined: %llu | parse %.3f s upload %.3f s kernels %.3f ms\n", (unsigned long long) st.pairs,
            (unsigned long long) st.combined, (unsigned long long) st.not_combined, st.ms_parse * 1e-3, st.ms_upload * 1e-3, st.ms_kernel);
    return KW(plasship_seqdb_write(ctx, r, c.pos.back().c_str())) || KW(plasship_seqdb_write(ctx, h, (c.pos.back() + "_h").c_str())) ? fail("mergereads") : EXIT_SUCCESS;
}

// ---- fused drivers: the iteration loop of a workflow script with every DB of the loop resident in HBM; only the first DB is read from disk and
//      only the last one written (plus, with --write-intermediate DIR, every iteration's assembly by a host thread on a second context while
//      the next iteration runs, with the workflow's .done sentinels) ----
static plasship_orf_params chainOrfParams(bool start, const Flags &f) {       // the two extractorfs passes (Assembler.cpp:116-130, GuidedNuclassembler.cpp:133-145)
    plasship_orf_params p; memset(&p, 0, sizeof(p));
    p.min_length = start ? 20 : 45; p.max_length = start ? 45 : 32734; p.max_gaps = 0; p.contig_start_mode = start ? 1 : 2; p.contig_end_mode = start ? 0 : 2;
    p.orf_start_mode = 0; p.forward_frames = 7; p.reverse_frames = 7; p.translation_table = f.translationTable; p.use_all_table_starts = f.allStarts; p.max_seq_len = 65535;
    return p;
}
// the input of a chain — a DB, FASTQ pairs (the workflows' mergereads step) or unpaired read files (their createdb step, data/assemble.sh:27-38) —
// as `in`, and the DB(s) iteration 0 starts from in L.db / L.aa.  `in` stays only where the guided tail needs the reads again.
static int prepareChainInput(Call &c, ChainLoop &L, SeqDb &in, bool keepReads, double &tRead) {
    plasship_ctx *ctx = c.ctx; const Flags &f = c.f; const char *mod = c.m->name;
    const bool prot = L.kind == CHAIN_PROTEIN, nuc = L.kind == CHAIN_NUCL, gd = L.kind == CHAIN_GUIDED;
    // a multi-GB input: the library takes its device arena (seconds of hipMalloc) while this thread reads and parses the DB files
    { struct stat stIn; if (stat(c.pos[0].c_str(), &stIn) == 0 && stIn.st_size >= ((off_t) 1 << 30)) (void) plasship_ctx_reserve_async(ctx); }
    const std::vector<const char *> files = cstrs(c.readFiles);
    if (!files.empty() && f.singleEnd) {       // the reads stay in HBM
        plasship_createdb_stats cs;
        if (K(plasship_createdb(ctx, files.data(), files.size(), nullptr, in.out(), &cs))) return fail(mod);
        fprintf(stdout, "createdb: %llu reads from %llu files\n", (unsigned long long) cs.entries, (unsigned long long) cs.files);
    } else if (!files.empty()) {               // the merged reads stay in HBM, the header DB is not needed
        SeqDb h(ctx); plasship_merge_stats ms;
        if (K(plasship_mergereads(ctx, files.data(), files.size(), nullptr, in.out(), h.out(), &ms))) return fail(mod);
        fprintf(stdout, "mergereads: %llu pairs, %llu combined\n", (unsigned long long) ms.pairs, (unsigned long long) ms.combined);
    } else if (K(plasship_seqdb_read(ctx, c.pos[0].c_str(), in.out()))) return fail(mod);
    tRead = now();
    const int dbtype = dbtypeOf(in);
    if (gd || (prot && (f.fromReads || dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES))) {
        if (dbtype != PLASSHIP_DBTYPE_NUCLEOTIDES) { fprintf(stdout, "%s: the input must be a nucleotide read DB\n", mod); return EXIT_FAILURE; }
        plasship_translate_params tp; tp.translation_table = f.translationTable; tp.add_orf_stop = 1; tp.max_seq_len = 65535;
        SeqDb ol(ctx), os(ctx); OrfHdr hl(ctx), hs(ctx); plasship_orf_stats ost;
        const plasship_orf_params pl = chainOrfParams(false, f), ps = chainOrfParams(true, f);
        if (K(extractOrfs(ctx, in, pl, ol.out(), hl.out(), &ost)) || K(extractOrfs(ctx, in, ps, os.out(), hs.out(), &ost))) return fail(mod);
        if (gd) {      // concatdbs of ORFs and headers, then one translatenucs (data/guidedNuclAssemble.sh:56-75): db = nucleotide ORFs, aa = their twins
            OrfHdr hh(ctx);
            if (K(plasship_seqdb_concat(ctx, ol, os, L.db.out())) || K(plasship_orfhdr_concat(ctx, hl, hs, hh.out())) || K(translateNucs(ctx, L.db, hh, tp, L.aa.out(), &ost))) return fail(mod);
        } else {       // translatenucs x2, then concatdbs (data/assemble.sh:41-77)
            SeqDb al(ctx), as(ctx);
            if (K(translateNucs(ctx, ol, hl, tp, al.out(), &ost)) || K(translateNucs(ctx, os, hs, tp, as.out(), &ost)) || K(plasship_seqdb_concat(ctx, al, as, L.db.out()))) return fail(mod);
        }
        if (!keepReads) in.reset();      // (the guided tail concatenates the reads: guidedNuclAssemble.sh:161-165)
    } else if ((prot && dbtype != PLASSHIP_DBTYPE_AMINO_ACIDS) || (nuc && dbtype != PLASSHIP_DBTYPE_NUCLEOTIDES)) {
        fprintf(stdout, "%s: wrong input DB type %d\n", mod, dbtype); return EXIT_FAILURE;
    } else L.db = std::move(in);
    return EXIT_SUCCESS;
}
static int runChain(Call &c) {
    plasship_ctx *ctx = c.ctx; const Flags &f = c.f; const char *mod = c.m->name; const int resumeFrom = c.resumeFrom;
    const bool prot = c.m->id == ASSEMBLE_CHAIN, nuc = c.m->id == NUCLASSEMBLE_CHAIN, gd = c.m->id == GUIDEDASSEMBLE_CHAIN;
    const std::vector<std::string> outs(c.pos.end() - nChainOut(c), c.pos.end());
    if (f.numIterations < 1) { fprintf(stdout, "--num-iterations must be at least 1\n"); return EXIT_FAILURE; }
    // a tail (--fasta-out; --db-mode 1 --db-out; --nuclassembly-out) needs SOURCE — the DB the loop starts from — and, on nucleotides,
    // every iteration's circular contigs: the loop keeps both
    const bool wantFasta = !f.fastaOut.empty(), wantDb = nuc && f.dbMode, wantNuclAsm = gd && !f.nuclAssemblyOut.empty();
    // The builders, and where the drivers differ from a module called with the same flags: no self matches; a backtrace on the guided chain only
    // (proteinaln2nucl reads it), whose extension works on nucleotides with the nucl half of --min-seq-id
    ChainLoop L(ctx, mod, prot ? CHAIN_PROTEIN : nuc ? CHAIN_NUCL : CHAIN_GUIDED, f);
    L.rp.add_backtrace = gd ? 1 : 0; L.rp.include_identity = 0;
    if (gd) L.ap.seq_id_thr = f.seqIdThrNucl;
    L.numIterations = f.numIterations; L.keepForTail = wantFasta || wantDb || wantNuclAsm; L.writeLastIntermediate = f.resume != 0;
    if (nuc) L.cyclePrefix = outs[0] + "_cycle_";
    L.intermediateName = gd ? "assembly_nucl_" : "assembly_";
    SeqDb in(ctx);
    // --write-intermediate: the writer thread reads the DB the loop holds in L.db while the next iteration runs.  It is declared AFTER every
    // handle it may read (L, in), so that on every return path joinOnExit runs first and the handles are released behind a writer that has
    // finished; the loop itself joins before it lets go of the DB the writer was given (runChainLoop).  Every exit path joins for two more
    // reasons: a joinable std::thread that goes out of scope terminates the process, and an intermediate DB must not be left half written
    // behind an ordinary error message.
    plasship_ctx *wctx = nullptr; std::thread writer; int writerRc = 0; std::string writerErr;
    struct JoinOnExit { std::thread &t; ~JoinOnExit() { if (t.joinable()) t.join(); } } joinOnExit{writer};
    if (!f.writeIntermediate.empty() && K(plasship_ctx_create(-1, &wctx))) return fail(mod);
    L.joinWriter = [&]() {
        if (writer.joinable()) writer.join();
        if (writerRc) fprintf(stdout, "%s: writing an intermediate DB failed: %s\n", mod, writerErr.c_str());
        return writerRc;
    };
    L.writeAsync = [&](const plasship_seqdb *d, const std::string &name) {
        if (!wctx) return;
        if (writer.joinable()) writer.join();       // (a failure of the write before this one is reported by the next joinWriter)
        const std::string path = f.writeIntermediate + "/" + name;
        writer = std::thread([&, d, path]() {
            if (plasship_seqdb_write(wctx, d, path.c_str())) { writerRc = 1; writerErr = plasship_last_error(); return; }      // (the error text is the writer THREAD's)
            FILE *fd = fopen((path + ".done").c_str(), "w"); if (fd) fclose(fd); else writerRc = 1;     // data/assemble.sh:147 `touch assembly_$STEP.done`
        });
    };
    if (f.resume && resumeFrom < 0 && !writeManifest(f.writeIntermediate + "/chain.manifest", c.manifest)) { fprintf(stdout, "%s: cannot write %s/chain.manifest\n", mod, f.writeIntermediate.c_str()); return EXIT_FAILURE; }
    // a resumed run reads DIR/assembly_<j> in place of the input; only a tail still needs the input, as SOURCE, made the way a fresh run makes it
    double tRead = now();
    if (resumeFrom < 0 || wantFasta || wantDb) if (const int rc = prepareChainInput(c, L, in, wantNuclAsm, tRead)) return rc;
    const double tPrep = now();
    if (resumeFrom >= 0) {
        // DIR/assembly_<j> is the DB iteration j handed to iteration j + 1: on nucleotides the rest after cyclecheck took the circular contigs out
        // (they are in <o>_cycle_<i>).  The library's caches (selected windows, positions, cyclecheck's "rest" lineage) start cold, as they do
        // for any DB read from files; none of them changes a result.
        const std::string from = f.writeIntermediate + "/" + L.intermediateName + std::to_string(resumeFrom);
        fprintf(stdout, "resuming at iteration %d (from %s)\n", resumeFrom + 1, from.c_str());
        L.startIteration = resumeFrom + 1; L.source = std::move(L.db);
        if (K(plasship_seqdb_read(ctx, from.c_str(), L.db.out()))) return fail(mod);
        const int dbtypeFrom = dbtypeOf(L.db);
        if (dbtypeFrom != (prot ? PLASSHIP_DBTYPE_AMINO_ACIDS : PLASSHIP_DBTYPE_NUCLEOTIDES)) { fprintf(stdout, "%s: wrong DB type %d of %s\n", mod, dbtypeFrom, from.c_str()); return EXIT_FAILURE; }
        // PREV_CYCLE_ALL of the tail: the circular contigs of the iterations up to j, from the files the interrupted run wrote next to its output
        for (int i = 0; nuc && L.keepForTail && i <= resumeFrom; i++) {
            const std::string cp = L.cyclePrefix + std::to_string(i);
            if (!isFile(cp) || !isFile(cp + ".index")) continue;       // (an iteration without circular contigs writes no file)
            SeqDb cyc(ctx), u(ctx);
            if (K(plasship_seqdb_read(ctx, cp.c_str(), cyc.out()))) return fail(mod);
            if (!L.cycAll) { L.cycAll = std::move(cyc); continue; }
            if (K(plasship_seqdb_concat_keys(ctx, L.cycAll, cyc, 1, u.out()))) return fail(mod);
            L.cycAll = std::move(u);
        }
    }
    L.tStart = tPrep;
    if (const int rc = runChainLoop(L)) return rc;
    const double tLoop = now();
    if (L.joinWriter()) return EXIT_FAILURE;
    if (KW(plasship_seqdb_write(ctx, L.db, outs[0].c_str())) || (gd && KW(plasship_seqdb_write(ctx, L.aa, outs[1].c_str())))) return fail(mod);
    if (wantFasta || wantDb) if (const int rc = chainTail(ctx, mod, nuc, L.db, std::move(L.source), std::move(L.cycAll), f, f.fastaOut, f.dbOut)) return rc;
    double tTail = 0;
    if (wantNuclAsm) {
        // ---- data/guidedNuclAssemble.sh:135-170 on the handles of the loop above ----
        const double tt0 = now();
        // `_only_assembled` (guidedNuclAssemble.sh:136-139): the entries of the last assembly_nucl_<i> whose key nucl_6f_start_long holds with a
        // shorter entry, `$3 > $6`; no length threshold — the nucleotide selection with only_extended and --min-contig-len 0 (include/plasship.h)
        plasship_select_params sp = {}; sp.mode = PLASSHIP_SELECT_NUCLEOTIDE; sp.only_extended = 1; sp.min_contig_len = 0;
        SeqDb only(ctx), mergedIn(ctx); plasship_select_stats ss;
        if (K(plasship_select_contigs(ctx, L.db, L.source, nullptr, &sp, only.out(), &ss))) return fail(mod);
        // concatdbs <only_assembled> <reads> guided_assembly.merged (guidedNuclAssemble.sh:161-165): the subset's keys are kept, the reads follow
        // from max(key) + 1 on in the order of their data file (DBConcat.cpp:63-118; 1 when nothing was selected: DBConcat.cpp:63,100)
        if (K(plasship_seqdb_concat(ctx, only, in, mergedIn.out()))) return fail(mod);
        size_t nAsm = 0, nMerged = 0; plasship_seqdb_info(L.db, &nAsm, nullptr, nullptr, nullptr, nullptr); plasship_seqdb_info(mergedIn, &nMerged, nullptr, nullptr, nullptr, nullptr);
        fprintf(stdout, "guided tail: %llu of %zu extended ORFs + the reads = %zu sequences\n", (unsigned long long) ss.n_selected, nAsm, nMerged);
        only.reset(); L.source.reset(); in.reset();
        // nuclassemble <merged> <out> --db-mode 1 (guidedNuclAssemble.sh:167-170) as penguin nuclassemble runs it (Nuclassembler.cpp:10-31), with the
        // nucleotide halves of the multi-parameters (GuidedNuclassembler.cpp:167-172): -k, --min-seq-id, --min-aln-len and the nucleotide scale (the
        // builder's, for CHAIN_NUCL); --cov-mode 0; no backtrace, no self matches; the extension as in the loop above
        ChainLoop N(ctx, mod, CHAIN_NUCL, f);
        N.kp.kmer_size = f.kNucl; N.kp.cov_mode = 0;
        N.rp.seq_id_thr = f.seqIdThrNucl; N.rp.min_aln_len = f.minAlnLenNucl; N.rp.cov_mode = 0; N.rp.add_backtrace = 0; N.rp.include_identity = 0;
        N.ap = L.ap;
        N.numIterations = f.numIterationsNucl; N.keepForTail = true;
        N.db = std::move(mergedIn); N.tStart = tt0;
        if (const int rc = runChainLoop(N)) return rc;
        if (const int rc = chainTail(ctx, mod, true, N.db, std::move(N.source), std::move(N.cycAll), f, std::string(), f.nuclAssemblyOut)) return rc;
        L.overlaps += N.overlaps; L.kernelMs += N.kernelMs;
        N.db.reset();        // (inside the tail's time)
        tTail = now() - tt0;
    }
    const double tEnd = now();
    fprintf(stdout, "chain: %d iterations, %llu candidate overlaps | read %.3fs preprocessing %.3fs iterations %.3fs (kernels %.3fs) write %.3fs", f.numIterations, L.overlaps,
            tRead - c.t0, tPrep - tRead, tLoop - tPrep, L.kernelMs * 1e-3, tEnd - tLoop - tTail);
    if (wantNuclAsm) fprintf(stdout, " nuclassembly (%d iterations) %.3fs", f.numIterationsNucl, tTail);
    fprintf(stdout, "\n");
    if (wctx) plasship_ctx_destroy(wctx);
    return EXIT_SUCCESS;
}

// ---- the modules.  Defaults: Parameters::setDefaults is Flags' own initialisers; kmermatcher adds setLinearFilterDefault (kmermatcher.cpp:566-573),
//      the fused drivers take their workflow's: src/workflow/Assembler.cpp:10-27 (plass assemble), Nuclassembler.cpp:10-31 (penguin nuclassemble),
//      GuidedNuclassembler.cpp:10-41 (penguin guided_nuclassemble, protein-guided stage) ----
static void chainDefaults(Flags &f) { f.alph = 13; f.kps = 60; f.ignoreMulti = 1; f.covThr = 0.0f; f.covMode = 0; f.evalThr = 1e-5; f.rescoreMode = 3; f.keepTarget = 1; f.hashShift = 67; }
static const Module kModules[] = {
    {"kmermatcher", KMERMATCHER, 2, "kmermatcher <i:sequenceDB> <o:prefDB>", [](Flags &f) { f.covThr = 0.8f; f.alph = 13; f.kps = 0; }, validateKmermatcher, runKmermatcher},
    {"rescorediagonal", RESCOREDIAGONAL, 4, "rescorediagonal <i:queryDB> <i:targetDB> <i:prefDB> <o:alnDB>", nullptr, validateRescorediagonal, runRescorediagonal},
    {"rescorediagonal-hamming", RESCOREDIAGONAL_HAMMING, 4, "rescorediagonal-hamming <i:queryDB> <i:targetDB> <i:prefDB> <o:prefDB>", nullptr, validateRescoreHamming, runRescoreHamming},
    {"rescorediagonal-local", RESCOREDIAGONAL_LOCAL, 4, "rescorediagonal-local <i:queryDB> <i:targetDB> <i:prefDB> <o:alnDB>", nullptr, validateRescoreLocal, runRescoreLocal},
    // linclust's greedy `clust` and its whole pre-cluster stage, lib/mmseqs/data/workflow/linclust.sh:21-57 (our own names: `clust` and `linclust` stay with the reference)
    {"clust-greedy", CLUST_GREEDY, 3, "clust-greedy <i:sequenceDB> <i:resultDB> <o:clusterDB>", nullptr, validateClustGreedy, runClust},
    // connected component under its own name, lib/mmseqs/data/workflow/linclust.sh:35,82 with --cluster-mode 1
    {"clust-connected", CLUST_CONNECTED, 3, "clust-connected <i:sequenceDB> <i:resultDB> <o:clusterDB>", nullptr, validateClustConnected, runClust},
    {"linclust-pre", LINCLUST_PRE, 3, "linclust-pre <i:sequenceDB> <o:preClusterDB> <o:prefilterDB>", [](Flags &f) { f.covThr = 0.8f; f.alph = 13; f.kps = 0; }, validateLinclustPre, runLinclustPre},
    {"mergeclusters-greedy", MERGECLUSTERS_GREEDY, 4, "mergeclusters-greedy <i:sequenceDB> <o:clusterDB> <i:clusterDB1> <i:clusterDB2>", nullptr, validateMergeclusters, runMergeclusters},
    {"linclust-ungapped", LINCLUST_UNGAPPED, 2, "linclust-ungapped <i:sequenceDB> <o:clusterDB>", [](Flags &f) { f.covThr = 0.8f; f.alph = 13; f.kps = 0; f.filterHits = 1; }, validateLinclustUngapped, runLinclustUngapped},
    // the protein workflow's filter step, the driver with it, and result2repseq (our own names: the reference's keep their answers)
    {"rescorediagonal-subst", RESCOREDIAGONAL_SUBST, 4, "rescorediagonal-subst <i:queryDB> <i:targetDB> <i:prefDB> <o:prefDB>", nullptr, validateRescoreSubst, runRescoreSubst},
    {"linclust-ungapped-prot", LINCLUST_UNGAPPED_PROT, 2, "linclust-ungapped-prot <i:sequenceDB> <o:clusterDB> [--rep-out DB]", [](Flags &f) { f.covThr = 0.8f; f.alph = 13; f.kps = 0; f.filterHits = 1; }, validateLinclustUngappedProt, runLinclustUngapped},
    {"clust-repseq", CLUST_REPSEQ, 3, "clust-repseq <i:sequenceDB> <i:clusterDB> <o:sequenceDB>", nullptr, nullptr, runClustRepseq},
    {"assembleresults", ASSEMBLERESULTS, 3, "assembleresults <i:sequenceDB> <i:alnResult> <o:reprSeqDB>", nullptr, nullptr, runAssembleresults},
    {"nuclassembleresults", NUCLASSEMBLERESULTS, 3, "nuclassembleresults <i:sequenceDB> <i:alnResult> <o:reprSeqDB>", nullptr, nullptr, runAssembleresults},
    {"guidedassembleresults", GUIDEDASSEMBLERESULTS, 5, "guidedassembleresults <i:nuclSequenceDB> <i:aaSequenceDB> <i:nuclAlnResult> <o:nuclAssembly> <o:aaAssembly>", nullptr, nullptr, runGuidedassembleresults},
    {"proteinaln2nucl", PROTEINALN2NUCL, 6, "proteinaln2nucl <i:queryNuclDB> <i:targetNuclDB> <i:queryAaDB> <i:targetAaDB> <i:alnDB> <o:alnDB>", nullptr, validateProteinaln2nucl, runProteinaln2nucl},
    {"findassemblystart", FINDASSEMBLYSTART, 3, "findassemblystart <i:sequenceDB> <i:alnDB> <o:sequenceDB>", nullptr, nullptr, runFindassemblystart},
    {"cyclecheck", CYCLECHECK, 2, "cyclecheck <i:sequenceDB> <o:sequenceDBcycle>", nullptr, nullptr, runCyclecheck},
    {"extractorfs", EXTRACTORFS, 2, "extractorfs <i:sequenceDB> <o:sequenceDB>", nullptr, nullptr, runExtractorfs},
    {"translatenucs", TRANSLATENUCS, 2, "translatenucs <i:sequenceDB> <o:sequenceDB>", nullptr, nullptr, runTranslatenucs},
    {"concatdbs", CONCATDBS, 3, "concatdbs <i:DB> <i:DB> <o:DB>", nullptr, validateConcatdbs, runConcatdbs},
    // the two with any genetic code of the reference (our own names: `extractorfs` and `translatenucs` keep their answers, the standard code only)
    {"extractorfs-gencode", EXTRACTORFS_GENCODE, 2, "extractorfs-gencode <i:sequenceDB> <o:sequenceDB> [--translation-table N] [--use-all-table-starts 1]", nullptr, validateGencode, runExtractorfs},
    {"translatenucs-gencode", TRANSLATENUCS_GENCODE, 2, "translatenucs-gencode <i:sequenceDB> <o:sequenceDB> [--translation-table N]", nullptr, validateGencode, runTranslatenucs},
    // the fused drivers (not reference modules: the iteration loops of data/assemble.sh:85-156, nuclassemble.sh:95-137 and guidedNuclAssemble.sh:77-126
    // with the DBs chained in HBM)
    {"assemble-chain", ASSEMBLE_CHAIN, 2, "assemble-chain: wrong number of databases",
     [](Flags &f) { chainDefaults(f); f.k = 14; f.scaleAA = 0.0f; f.seqIdThr = 0.9f; f.maxSeqLen = 65535; f.numIterations = 12; }, validateChain, runChain},
    {"nuclassemble-chain", NUCLASSEMBLE_CHAIN, 2, "nuclassemble-chain: wrong number of databases",
     [](Flags &f) { chainDefaults(f); f.k = 22; f.scaleNucl = 0.1f; f.seqIdThr = 0.99f; f.maxSeqLen = 200000; f.numIterations = 8; f.onlyExt = 1; f.chopCycle = 1; }, validateChain, runChain},
    {"guidedassemble-chain", GUIDEDASSEMBLE_CHAIN, 3, "guidedassemble-chain: wrong number of databases",
     [](Flags &f) { chainDefaults(f); f.k = 14; f.scaleAA = 0.1f; f.scaleNucl = 0.1f; f.seqIdThr = 0.97f; f.maxSeqLen = 200000; f.numIterations = 5; f.onlyExt = 1; f.covMode = 1; f.addBt = 1; },
     validateChain, runChain},
    // createdb on the device for read files (our own name, like the chains: `createdb` itself stays with the reference)
    {"createdb-reads", CREATEDB_READS, 0, "createdb-reads <i:file1[.gz]> ... <i:fileN[.gz]> <o:sequenceDB>", nullptr, validateCreatedbReads, runCreatedbReads},
    // (flags: the reference's onlythreads set, plass.cpp:47, Parameters.cpp:301-303: --threads, -v)
    {"mergereads", MERGEREADS, 0, "mergereads <i:fastqFile1[.gz]> <i:fastqFile2[.gz]> ... <o:sequenceDB>", nullptr, validateMergereads, runMergereads},
};
static const char kUsage[] =
    "usage: plass-hip <kmermatcher|rescorediagonal|assembleresults|nuclassembleresults|guidedassembleresults|proteinaln2nucl|findassemblystart|"
    "cyclecheck|extractorfs|translatenucs|concatdbs> <dbs…> [flags]\n"
    "       plass-hip mergereads <i:r1.fastq[.gz]> <i:r2.fastq[.gz]> [<r1b> <r2b> …] <o:readDB>      (writes <o> and <o>_h)\n"
    "       plass-hip assemble-chain <i:fragmentDB|readDB | r1.fastq r2.fastq …> <o:assemblyDB> [--num-iterations 12] [--from-reads 1] [--write-intermediate DIR]\n"
    "       plass-hip nuclassemble-chain <i:nuclDB | r1.fastq r2.fastq …> <o:assemblyDB> [--num-iterations 8]        (writes <o>_cycle_<i> for circular contigs)\n"
    "       (assemble-chain --filter-proteins 0 / nuclassemble-chain [--min-contig-len 1000] [--contig-output-mode 1]: --fasta-out FILE writes the\n"
    "        selected contigs as FASTA, the workflows' tail, data/assemble.sh:159-201, data/nuclassemble.sh:138-207)\n"
    "       (nuclassemble-chain --db-mode 1 --db-out DB: the selected contigs as DB, DB.index, DB.dbtype and DB_cycle.index instead, nuclassemble.sh:200-207)\n"
    "       plass-hip guidedassemble-chain <i:readDB | r1.fastq r2.fastq …> <o:nuclAssemblyDB> <o:aaAssemblyDB> [--num-iterations aa:5,nucl:5]\n"
    "       (--nuclassembly-out DB: goes on with data/guidedNuclAssemble.sh:135-170 — the extended ORFs + the reads through nuclassemble --db-mode 1)\n"
    "       (assemble-chain / nuclassemble-chain --write-intermediate DIR --resume 1: go on behind the highest complete DIR/assembly_<i> of an\n"
    "        earlier run, the workflows' .done sentinels, data/assemble.sh:86-147; DIR/chain.manifest holds the parameters and the input it may go on with)\n"
    "       (FASTQ pairs: merged on the GPU first, as the workflows' mergereads step, data/assemble.sh:27-38)\n"
    "       (--single-end 1 on the three chains: every file before the output(s) is an unpaired FASTQ / FASTA read file, the workflows' createdb step)\n"
    "       plass-hip createdb-reads <i:file[.gz]> [<i:file2> …] <o:readDB> [--shuffle 1] [--id-offset 0] [--dbtype 0]   (writes <o>, <o>_h, <o>.lookup, <o>.source)\n";

// the command line behind the module's name into c.pos and c.f: 0, or the exit code
static int parseArgs(int argc, char **argv, Call &c) {
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (!(a.size() > 1 && a[0] == '-' && !(a[1] >= '0' && a[1] <= '9'))) { c.pos.push_back(a); continue; }     // ("-5" is a positional)
        const Flag *fl = nullptr;
        for (const Flag &k : kFlags) if (a == k.name && (k.owners & c.m->id)) fl = &k;
        if (!fl) { fprintf(stdout, "Unrecognized parameter \"%s\" for module %s\n", a.c_str(), c.m->name); return EXIT_FAILURE; }
        std::string v; bool haveValue = true;
        if (fl->kind == BOOL || fl->kind == ZERO_BOOL) {
            if (i + 1 >= argc || argv[i + 1][0] == '-') haveValue = false; else v = argv[++i];
        } else {
            if (i + 1 >= argc) { fprintf(stdout, "Missing argument %s\n", a.c_str()); return EXIT_FAILURE; }
            v = argv[++i];
        }
        c.f.seen.insert(a);
        if (const int rc = applyFlag(*fl, c.f, c.m->id, v, haveValue)) return rc;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { fputs(kUsage, stdout); return EXIT_FAILURE; }
    Call c;
    for (const Module &m : kModules) if (!strcmp(argv[1], m.name)) c.m = &m;
    if (!c.m) return unsupported("plass-hip: module \"%s\" is not part of the GPU hot path (use the reference binary for it)\n", argv[1]);
    if (c.m->defaults) c.m->defaults(c.f);
    if (const int rc = parseArgs(argc, argv, c)) return rc;
    if (c.m->validate) if (const int rc = c.m->validate(c)) return rc;
    const char *dry = getenv("PLASSHIP_CLI_DRYRUN"); const int dryLevel = dry ? atoi(dry) : 0;
    if (dryLevel != 0) {
        fprintf(stdout, "plass-hip dry run: %s accepted (%zu positional arguments, %zu flags); nothing read or computed\n", c.m->name, c.pos.size(), c.f.seen.size());
        if (dryLevel == 2) for (const auto &m : kMembers) fprintf(stdout, "flag.%s %s\n", m.name, m.dest.str(c.f).c_str());
        return EXIT_DRYRUN_ACCEPTED;
    }
    if (K(plasship_ctx_create(-1, &c.ctx))) return fail("plass-hip");
    c.t0 = now();
    if (c.m->nPos && c.pos.size() != c.m->nPos && c.readFiles.empty()) { fprintf(stdout, "%s\n", c.m->usage); return EXIT_FAILURE; }
    if (const int rc = c.m->run(c)) return rc;
    fprintf(stdout, "Time for processing: %.3fs\n", now() - c.t0);
    // Every output DB is complete and renamed into place by now, and every handle released.  Taking the context apart — unmapping an arena of up to
    // 270 GB, the runtime's own shutdown — is work the driver does for an exiting process anyway; a command-line tool leaves it to it (round 6: ~1 s
    // of the fused driver's wall clock at 50 M reads).  PLASSHIP_CLI_FULL_TEARDOWN=1: the orderly way (leak checkers).
    fflush(stdout); fflush(stderr);
    if (!getenv("PLASSHIP_CLI_FULL_TEARDOWN")) _exit(EXIT_SUCCESS);
    plasship_ctx_destroy(c.ctx);
    return EXIT_SUCCESS;
}
