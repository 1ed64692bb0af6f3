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
#include <chrono>
#include <unistd.h>
#include <cstdarg>
#include <climits>
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
    std::set<std::string> seen;
};

// Exit codes beyond EXIT_SUCCESS / EXIT_FAILURE: a request that is well-formed for the REFERENCE module but lies
// outside what the GPU path implements (--rescore-mode 0, --wrapped-scoring 1, masking, spaced k-mers, automatic -k, a module that is not
// part of the hot path, PLASSHIP_ERR_UNSUPPORTED from the library) ends with EXIT_UNSUPPORTED before anything is written, so that a
// wrapper can hand exactly that call to the reference binary: `linclust` at the end of `penguin guided_nuclassemble` calls
// `rescorediagonal --rescore-mode 0 --wrapped-scoring 1` (lib/mmseqs/data/workflow/linclust.sh:30) through the same $MMSEQS.
// EXIT_DRYRUN_ACCEPTED: with PLASSHIP_CLI_DRYRUN=1 the command line is parsed and validated, nothing is read or computed (no GPU needed) —
// what tools/workflow_dropin_check.sh uses to exercise the routing of every call the unmodified workflow scripts make.
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

// ---- the iteration loop of a workflow script (data/assemble.sh:85-156, nuclassemble.sh:95-137, guidedNuclAssemble.sh:77-126) with every DB of
//      the loop resident in HBM.  One function for the three drivers and for the nuclassemble that guidedassemble-chain --nuclassembly-out
//      runs on the merged DB (guidedNuclAssemble.sh:167-170). ----
enum ChainKind { CHAIN_PROTEIN, CHAIN_NUCL, CHAIN_GUIDED };
struct ChainLoop {
    plasship_ctx *ctx = nullptr; const char *name = ""; ChainKind kind = CHAIN_PROTEIN;
    int numIterations = 1, startIteration = 0, k = 0, alph = 13, kps = 60, ignoreMulti = 1, covMode = 0, hashShift = 67, gapOpenNucl = 5, gapExtendNucl = 2, chopCycle = 1;
    float kpsScale = 0.0f, covThr = 0.0f; unsigned long long maxSeqLen = 65535;
    plasship_rescore_params rp; plasship_assemble_params ap;
    bool keepForTail = false;            // keep SOURCE and every iteration's circular contigs: a tail follows
    std::string cyclePrefix;             // nucleotide: circular contigs of iteration i are written to <cyclePrefix><i> ("": they are not)
    std::string intermediateName;        // --write-intermediate: "assembly_" / "assembly_nucl_" ("": nothing is written)
    bool writeLastIntermediate = false;  // --resume 1: the last iteration's DB is a resume point too (a finished run can be extended)
    std::function<int()> joinWriter; std::function<void(const plasship_seqdb *, const std::string &)> writeAsync;
    // in: the DB(s) iteration startIteration starts from; out: the last iteration's
    plasship_seqdb *db = nullptr, *aa = nullptr;
    // keepForTail: SOURCE of the tail, PREV_CYCLE_ALL (nullptr: no circular contig).  A loop that starts at iteration 0 sets both; one that
    // starts later (--resume 1) is handed what the iterations before startIteration would have left here
    plasship_seqdb *source = nullptr, *cycAll = nullptr;
    unsigned long long overlaps = 0; double kernelMs = 0, tStart = 0;
};
static int runChainLoop(ChainLoop &L) {
    plasship_ctx *ctx = L.ctx;
    const bool prot = L.kind == CHAIN_PROTEIN, nuc = L.kind == CHAIN_NUCL, gd = L.kind == CHAIN_GUIDED;
    plasship_seqdb *&db = L.db, *&aa = L.aa, *&source = L.source, *&cycAll = L.cycAll;
    // SOURCE is the DB the loop starts from (the reads; the guided chain's nucl_6f_start_long; the fragments before findassemblystart: kept below)
    if (L.keepForTail && !prot && !source) source = db;
    for (int it = L.startIteration; it < L.numIterations; it++) {
        plasship_kmermatch_params kp; memset(&kp, 0, sizeof(kp));
        kp.kmer_size = L.k; kp.alphabet_size = L.alph; kp.kmers_per_seq = L.kps; kp.kmers_per_seq_scale = L.kpsScale; kp.ignore_multi_kmer = L.ignoreMulti;
        kp.cov_mode = L.covMode; kp.cov_thr = L.covThr;
        // plass assemble: --hash-shift grows with every second iteration, iteration 0 keeps non-extendable matches (Assembler.cpp:99-110)
        // (67, 68, 68, 69, …: a function of the iteration's index, wherever this loop starts)
        if (prot) { kp.hash_shift = L.hashShift + (it + 1) / 2; kp.include_only_extendable = it > 0; } else { kp.hash_shift = L.hashShift; kp.include_only_extendable = 1; }
        plasship_seqdb *q = gd ? aa : db;
        plasship_cands *c = nullptr; plasship_alns *al = nullptr; plasship_kmermatch_stats ks; plasship_rescore_stats rs; plasship_assemble_stats as;
        if (K(plasship_kmermatch(ctx, q, &kp, &c, &ks)) || K(plasship_rescore(ctx, q, q, c, &L.rp, &al, &rs))) return fail(L.name);
        if (prot && it == 0) {         // data/assemble.sh:110-141: findassemblystart, then k-mer matching and re-scoring again on the corrected sequences
            plasship_seqdb *corr = nullptr; plasship_findstart_stats fs;
            if (K(plasship_find_assembly_start(ctx, db, al, &corr, &fs))) return fail(L.name);
            plasship_alns_free(ctx, al); plasship_cands_free(ctx, c);
            if (L.keepForTail) source = db; else plasship_seqdb_free(ctx, db);      // SOURCE of the tail: aa_6f_start_long, before the correction
            db = corr; q = db;
            if (K(plasship_kmermatch(ctx, q, &kp, &c, &ks)) || K(plasship_rescore(ctx, q, q, c, &L.rp, &al, &rs))) return fail(L.name);
        }
        L.overlaps += ks.n_candidates; L.kernelMs += ks.ms_extract + ks.ms_sort1 + ks.ms_group + ks.ms_sort2 + ks.ms_reduce + rs.ms_kernel;
        plasship_seqdb *next = nullptr, *nextAa = nullptr;
        if (gd) {
            plasship_alns *na = nullptr; plasship_aln2nucl_params np; np.gap_open = L.gapOpenNucl; np.gap_extend = L.gapExtendNucl; plasship_aln2nucl_stats ns;
            if (K(plasship_aln2nucl(ctx, db, db, aa, aa, al, &np, &na, &ns)) || K(plasship_guided_assemble(ctx, db, aa, na, &L.ap, &next, &nextAa, &as))) return fail(L.name);
            plasship_alns_free(ctx, na);
        } else if (K(plasship_assemble(ctx, db, al, &L.ap, &next, &as))) return fail(L.name);
        L.kernelMs += as.ms_kernel;
        plasship_alns_free(ctx, al); plasship_cands_free(ctx, c);
        if (L.joinWriter && L.joinWriter()) return EXIT_FAILURE;   // the writer read `db` (the caller's joinWriter prints the message)
        if (db != source) plasship_seqdb_free(ctx, db);
        if (gd) plasship_seqdb_free(ctx, aa);
        db = next; aa = nextAa;
        if (nuc) {     // data/nuclassemble.sh:19-61,132: circular contigs leave the loop, the rest goes on
            plasship_seqdb *cyc = nullptr, *rest = nullptr; plasship_cyclecheck_params cp; cp.max_seq_len = L.maxSeqLen; cp.chop_cycle = L.chopCycle; plasship_cyclecheck_stats cs;
            if (K(plasship_cyclecheck(ctx, db, &cp, &cyc, &rest, &cs))) return fail(L.name);
            if (cs.n_cyclic && !L.cyclePrefix.empty() && KW(plasship_seqdb_write(ctx, cyc, (L.cyclePrefix + std::to_string(it)).c_str()))) return fail(L.name);
            if (L.keepForTail && cs.n_cyclic) {       // PREV_CYCLE_ALL: every iteration's circular contigs (nuclassemble.sh:35-41, concatdbs --preserve-keys)
                if (!cycAll) { cycAll = cyc; cyc = nullptr; }
                else { plasship_seqdb *u = nullptr; if (K(plasship_seqdb_concat_keys(ctx, cycAll, cyc, 1, &u))) return fail(L.name); plasship_seqdb_free(ctx, cycAll); cycAll = u; }
            }
            if (cyc) plasship_seqdb_free(ctx, cyc);
            plasship_seqdb_free(ctx, db); db = rest;
        }
        fprintf(stdout, "iteration %d: candidates %llu verified %llu extended %llu (%.3f s since the DB was read)\n", it, (unsigned long long) ks.n_candidates, (unsigned long long) rs.n_accepted, (unsigned long long) as.n_extended, now() - L.tStart);
        if ((it + 1 < L.numIterations || L.writeLastIntermediate) && L.writeAsync && !L.intermediateName.empty()) L.writeAsync(db, L.intermediateName + std::to_string(it));
    }
    return EXIT_SUCCESS;
}
// ---- the workflows' tail on the last DB of a loop (data/assemble.sh:159-201, nuclassemble.sh:138-207): RESULT, the `_only_assembled` selection,
//      then FASTA (fastaOut) or, in db-mode, the DB of the selected contigs and its cycle index (dbOut).  Frees source and cycAll. ----
static int chainTail(plasship_ctx *ctx, const char *name, bool nuc, plasship_seqdb *db, plasship_seqdb *source, plasship_seqdb *cycAll,
                     int contigOutputMode, int minContigLen, const std::string &fastaOut, const std::string &dbOut) {
    // RESULT: the last assembly, or (nucleotide, circular contigs found) the non-circular rest + every circular contig (nuclassemble.sh:140-148)
    plasship_seqdb *result = db, *merged = nullptr, *sel = nullptr;
    if (cycAll) { if (K(plasship_seqdb_concat_keys(ctx, db, cycAll, 1, &merged))) return fail(name); result = merged; }
    plasship_select_params sp; memset(&sp, 0, sizeof(sp));
    sp.mode = nuc ? PLASSHIP_SELECT_NUCLEOTIDE : PLASSHIP_SELECT_PROTEIN; sp.only_extended = contigOutputMode == 1; sp.min_contig_len = minContigLen;
    plasship_select_stats ss;
    if (!source) { fprintf(stdout, "%s: the tail needs the fragment DB before findassemblystart\n", name); return EXIT_FAILURE; }
    if (K(plasship_select_contigs(ctx, result, source, cycAll, &sp, &sel, &ss))) return fail(name);
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
    plasship_seqdb_free(ctx, sel); if (merged) plasship_seqdb_free(ctx, merged); if (cycAll) plasship_seqdb_free(ctx, cycAll);
    plasship_seqdb_free(ctx, source);
    return EXIT_SUCCESS;
}

// ---- --resume 1: the resume points --write-intermediate DIR leaves (DIR/assembly_<i> + DIR/assembly_<i>.done, data/assemble.sh:147) and
//      DIR/chain.manifest, the parameters and the input they were computed with ----
static bool isFile(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
// the highest i < numIterations whose sentinel and DB files exist (the sentinel is touched after the DB is complete); -1: none
static int resumePoint(const std::string &dir, const std::string &name, int numIterations) {
    for (int i = numIterations - 1; i >= 0; i--) {
        const std::string p = dir + "/" + name + std::to_string(i);
        if (isFile(p + ".done") && isFile(p) && isFile(p + ".index") && isFile(p + ".dbtype")) return i;
    }
    return -1;
}
typedef std::vector<std::pair<std::string, std::string>> Manifest;
static std::string fmtNum(const char *fmt, ...) { char b[96]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof(b), fmt, ap); va_end(ap); return b; }
// what a continuation must share with the run that wrote the resume points: the module, every parameter the loop's result depends on (keyed
// by its flag) and the input files.  Not --num-iterations, the outputs or the tail's flags: those may differ.
static Manifest chainManifest(const std::string &mod, const Flags &f, const std::vector<std::string> &inputs) {
    Manifest m;
    m.emplace_back("module", mod);
    m.emplace_back("-k", std::to_string(f.k));
    m.emplace_back("--alph-size", std::to_string(f.alph));
    m.emplace_back("--kmer-per-seq", std::to_string(f.kps));
    m.emplace_back("--kmer-per-seq-scale", fmtNum("%.9g", (double) (mod == "nuclassemble-chain" ? f.scaleNucl : f.scaleAA)));
    m.emplace_back("--hash-shift", std::to_string(f.hashShift));
    m.emplace_back("--min-seq-id", fmtNum("%.9g", (double) f.seqIdThr));
    m.emplace_back("-e", fmtNum("%.17g", f.evalThr));
    m.emplace_back("-c", fmtNum("%.9g", (double) f.covThr));
    m.emplace_back("--cov-mode", std::to_string(f.covMode));
    m.emplace_back("--min-aln-len", std::to_string(f.minAlnLen));
    m.emplace_back("--seq-id-mode", std::to_string(f.seqIdMode));
    m.emplace_back("--rescore-mode", std::to_string(f.rescoreMode));
    m.emplace_back("--ignore-multi-kmer", std::to_string(f.ignoreMulti));
    m.emplace_back("--include-only-extendable", std::to_string(f.onlyExt));
    m.emplace_back("--keep-target", std::to_string(f.keepTarget));
    m.emplace_back("--max-seq-len", std::to_string(f.maxSeqLen));
    m.emplace_back("--chop-cycle", std::to_string(f.chopCycle));
    m.emplace_back("--from-reads", std::to_string(f.fromReads));
    m.emplace_back("--single-end", std::to_string(f.singleEnd));
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

// which flags a module owns (its parameter vector in the reference)
static const std::map<std::string, std::set<std::string>> &moduleFlags() {
    static const std::set<std::string> common = {"--threads", "-v", "--compressed"};
    static std::map<std::string, std::set<std::string>> m;
    if (m.empty()) {
        m["kmermatcher"] = {"--sub-mat", "--alph-size", "--min-seq-id", "--kmer-per-seq", "--spaced-kmer-mode", "--spaced-kmer-pattern", "--kmer-per-seq-scale",
                            "--adjust-kmer-len", "--mask", "--mask-lower-case", "--cov-mode", "-k", "-c", "--max-seq-len", "--hash-shift", "--split-memory-limit",
                            "--include-only-extendable", "--ignore-multi-kmer"};
        m["rescorediagonal"] = {"--sub-mat", "--rescore-mode", "--wrapped-scoring", "--filter-hits", "-e", "-c", "-a", "--cov-mode", "--min-seq-id", "--min-aln-len",
                                "--seq-id-mode", "--add-self-matches", "--sort-results", "--db-load-mode"};
        m["assembleresults"] = {"--min-seq-id", "--max-seq-len", "--keep-target", "--rescore-mode"};
        m["nuclassembleresults"] = m["assembleresults"];
        m["guidedassembleresults"] = m["assembleresults"];
        m["proteinaln2nucl"] = {"--sub-mat", "--gap-open", "--gap-extend"};
        m["findassemblystart"] = {};
        m["cyclecheck"] = {"--max-seq-len", "--chop-cycle"};
        m["extractorfs"] = {"--min-length", "--max-length", "--max-gaps", "--contig-start-mode", "--contig-end-mode", "--orf-start-mode", "--forward-frames",
                            "--reverse-frames", "--translation-table", "--translate", "--use-all-table-starts", "--id-offset", "--create-lookup"};
        m["translatenucs"] = {"--translation-table", "--add-orf-stop"};
        m["concatdbs"] = {"--preserve-keys", "--take-larger-entry"};
        // the fused drivers (not reference modules: the iteration loops of data/assemble.sh:85-156, nuclassemble.sh:95-137 and
        // guidedNuclAssemble.sh:77-126 with the DBs chained in HBM); flags = the workflow's own, defaults = the workflow's
        m["assemble-chain"] = {"--num-iterations", "--write-intermediate", "--from-reads", "-k", "--alph-size", "--kmer-per-seq", "--kmer-per-seq-scale", "--min-seq-id", "-e", "-c",
                               "--cov-mode", "--max-seq-len", "--keep-target", "--hash-shift", "--ignore-multi-kmer", "--rescore-mode", "--min-aln-len", "--seq-id-mode"};
        m["guidedassemble-chain"] = m["assemble-chain"];
        // (--nuclassembly-out DB: the nuclassemble of data/guidedNuclAssemble.sh:135-170 behind the guided loop, with the nucleotide workflow's own flags)
        m["guidedassemble-chain"].insert({"--nuclassembly-out", "--chop-cycle", "--min-contig-len", "--contig-output-mode"});
        m["nuclassemble-chain"] = m["assemble-chain"]; m["nuclassemble-chain"].insert({"--chop-cycle", "--fasta-out", "--min-contig-len", "--contig-output-mode", "--db-mode", "--db-out"});
        m["assemble-chain"].insert({"--fasta-out", "--filter-proteins", "--protein-filter-threshold"});
        for (const char *c : {"assemble-chain", "nuclassemble-chain", "guidedassemble-chain"}) m[c].insert({"--single-end", "--resume"});
        // createdb on the device for read files (our own name, like the chains: `createdb` itself stays with the reference); createdb's flags
        m["createdb-reads"] = {"--shuffle", "--id-offset", "--dbtype", "--createdb-mode", "--write-lookup"};
        m["mergereads"] = {};       // the reference's onlythreads set (plass.cpp:47, Parameters.cpp:301-303): --threads, -v
        for (auto &kv : m) kv.second.insert(common.begin(), common.end());
    }
    return m;
}
// bool-typed parameters of the reference (typeid(bool)): a missing value toggles the default (Parameters.cpp:1670-1677)
static const std::set<std::string> &boolFlags() {
    static const std::set<std::string> b = {"-a", "--add-self-matches", "--wrapped-scoring", "--filter-hits", "--include-only-extendable", "--ignore-multi-kmer",
                                            "--keep-target", "--chop-cycle", "--adjust-kmer-len", "--use-all-table-starts", "--add-orf-stop", "--preserve-keys",
                                            "--take-larger-entry", "--db-mode", "--shuffle"};
    return b;
}
static bool parseBool(const std::string &v, bool &ok) {                 // Parameters::parseBool: TRUE/1 | FALSE/0
    ok = true;
    if (v == "1" || v == "TRUE" || v == "true") return true;
    if (v == "0" || v == "FALSE" || v == "false") return false;
    ok = false; return false;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stdout, "usage: plass-hip <kmermatcher|rescorediagonal|assembleresults|nuclassembleresults|guidedassembleresults|proteinaln2nucl|findassemblystart|"
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
                        "       plass-hip createdb-reads <i:file[.gz]> [<i:file2> …] <o:readDB> [--shuffle 1] [--id-offset 0] [--dbtype 0]   (writes <o>, <o>_h, <o>.lookup, <o>.source)\n");
        return EXIT_FAILURE;
    }
    const std::string mod = argv[1];
    const auto mf = moduleFlags().find(mod);
    if (mf == moduleFlags().end()) {
        return unsupported("plass-hip: module \"%s\" is not part of the GPU hot path (use the reference binary for it)\n", mod.c_str());
    }
    Flags f; std::vector<std::string> pos;
    if (mod == "kmermatcher") { f.covThr = 0.8f; f.alph = 13; f.kps = 0; }                    // setLinearFilterDefault
    const bool chain = mod == "assemble-chain" || mod == "nuclassemble-chain" || mod == "guidedassemble-chain";
    if (chain) {
        // the workflows' defaults: src/workflow/Assembler.cpp:10-27 (plass assemble), Nuclassembler.cpp:10-31 (penguin nuclassemble),
        // GuidedNuclassembler.cpp:10-41 (penguin guided_nuclassemble, protein-guided stage)
        f.alph = 13; f.kps = 60; f.ignoreMulti = 1; f.covThr = 0.0f; f.covMode = 0; f.evalThr = 1e-5; f.rescoreMode = 3; f.keepTarget = 1; f.hashShift = 67;
        if (mod == "assemble-chain") { f.k = 14; f.scaleAA = 0.0f; f.seqIdThr = 0.9f; f.maxSeqLen = 65535; f.numIterations = 12; }
        else if (mod == "nuclassemble-chain") { f.k = 22; f.scaleNucl = 0.1f; f.seqIdThr = 0.99f; f.maxSeqLen = 200000; f.numIterations = 8; f.onlyExt = 1; f.chopCycle = 1; }
        else { f.k = 14; f.scaleAA = 0.1f; f.scaleNucl = 0.1f; f.seqIdThr = 0.97f; f.maxSeqLen = 200000; f.numIterations = 5; f.onlyExt = 1; f.covMode = 1; f.addBt = 1; }
    }
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        if (!(a.size() > 1 && a[0] == '-' && !(a[1] >= '0' && a[1] <= '9'))) { pos.push_back(a); continue; }
        if (!mf->second.count(a)) { fprintf(stdout, "Unrecognized parameter \"%s\" for module %s\n", a.c_str(), mod.c_str()); return EXIT_FAILURE; }
        std::string v, t; bool haveValue = true;
        if (boolFlags().count(a)) {
            if (i + 1 >= argc || argv[i + 1][0] == '-') haveValue = false; else v = argv[++i];
        } else {
            if (i + 1 >= argc) { fprintf(stdout, "Missing argument %s\n", a.c_str()); return EXIT_FAILURE; }
            v = argv[++i];
        }
        f.seen.insert(a);
        auto setBool = [&](int &field) -> bool {
            if (!haveValue) { field = !field; return true; }
            bool ok; const bool b = parseBool(v, ok);
            if (!ok) { fprintf(stdout, "Error in argument %s\n", a.c_str()); return false; }
            field = b ? 1 : 0; return true;
        };
        if (a == "-k") {       // (guided chain: a MultiParam, one value sets both halves — lib/mmseqs/src/commons/MultiParam.cpp:23-39)
            if (mod == "guidedassemble-chain") { if (multiParam(v, "aa", t)) f.k = atoi(t.c_str()); if (multiParam(v, "nucl", t)) f.kNucl = atoi(t.c_str()); }
            else f.k = atoi(v.c_str());
        }
        else if (a == "--num-iterations") {
            std::string t2; f.numIterations = atoi((multiParam(v, mod == "assemble-chain" || mod == "guidedassemble-chain" ? "aa" : "nucl", t2) ? t2 : v).c_str());
            if (multiParam(v, "nucl", t2)) f.numIterationsNucl = atoi(t2.c_str());
        }
        else if (a == "--nuclassembly-out") f.nuclAssemblyOut = v;
        else if (a == "--db-out") f.dbOut = v;
        else if (a == "--db-mode") { if (!setBool(f.dbMode)) return EXIT_FAILURE; }
        else if (a == "--write-intermediate") f.writeIntermediate = v;
        else if (a == "--fasta-out") f.fastaOut = v;
        else if (a == "--filter-proteins") f.filterProteins = atoi(v.c_str());
        else if (a == "--protein-filter-threshold") { /* filternoncoding's threshold: only read by the step --filter-proteins 1 runs */ }
        else if (a == "--min-contig-len") f.minContigLen = atoi(v.c_str());
        else if (a == "--contig-output-mode") f.contigOutputMode = atoi(v.c_str());
        else if (a == "--from-reads") f.fromReads = atoi(v.c_str());
        else if (a == "--resume") f.resume = atoi(v.c_str());
        else if (a == "--alph-size") { if (multiParam(v, "aa", t)) f.alph = atoi(t.c_str()); }
        else if (a == "--kmer-per-seq") f.kps = atoi(v.c_str());
        else if (a == "--kmer-per-seq-scale") { if (multiParam(v, "aa", t)) f.scaleAA = strtof(t.c_str(), nullptr); if (multiParam(v, "nucl", t)) f.scaleNucl = strtof(t.c_str(), nullptr); }
        else if (a == "--hash-shift") f.hashShift = atoi(v.c_str());
        else if (a == "--include-only-extendable") { if (!setBool(f.onlyExt)) return EXIT_FAILURE; }
        else if (a == "--ignore-multi-kmer") { if (!setBool(f.ignoreMulti)) return EXIT_FAILURE; }
        else if (a == "--cov-mode") f.covMode = atoi(v.c_str());
        else if (a == "-c") f.covThr = strtof(v.c_str(), nullptr);
        else if (a == "--rescore-mode") f.rescoreMode = atoi(v.c_str());
        else if (a == "-e") f.evalThr = strtod(v.c_str(), nullptr);
        else if (a == "--min-seq-id") {
            if (mod == "guidedassemble-chain") { if (multiParam(v, "aa", t)) f.seqIdThr = strtof(t.c_str(), nullptr); if (multiParam(v, "nucl", t)) f.seqIdThrNucl = strtof(t.c_str(), nullptr); }
            else if (mod == "nuclassemble-chain") { if (multiParam(v, "nucl", t)) f.seqIdThr = strtof(t.c_str(), nullptr); }
            else if (mod == "assemble-chain") { if (multiParam(v, "aa", t)) f.seqIdThr = strtof(t.c_str(), nullptr); }
            else f.seqIdThr = strtof(v.c_str(), nullptr);
        }
        else if (a == "--min-aln-len") {
            if (mod == "guidedassemble-chain") { if (multiParam(v, "aa", t)) f.minAlnLen = atoi(t.c_str()); if (multiParam(v, "nucl", t)) f.minAlnLenNucl = atoi(t.c_str()); }
            else f.minAlnLen = atoi(v.c_str());
        }
        else if (a == "--seq-id-mode") f.seqIdMode = atoi(v.c_str());
        else if (a == "-a") { if (!setBool(f.addBt)) return EXIT_FAILURE; }
        else if (a == "--add-self-matches") { if (!setBool(f.addSelf)) return EXIT_FAILURE; }
        else if (a == "--max-seq-len") f.maxSeqLen = strtoull(v.c_str(), nullptr, 10);
        else if (a == "--chop-cycle") { if (!setBool(f.chopCycle)) return EXIT_FAILURE; }
        else if (a == "--keep-target") { if (!setBool(f.keepTarget)) return EXIT_FAILURE; }
        else if (a == "--gap-open") { if (multiParam(v, "nucl", t)) f.gapOpenNucl = atoi(t.c_str()); }
        else if (a == "--gap-extend") { if (multiParam(v, "nucl", t)) f.gapExtendNucl = atoi(t.c_str()); }
        else if (a == "--wrapped-scoring") { if (!setBool(f.wrapped)) return EXIT_FAILURE; }
        else if (a == "--filter-hits") { if (!setBool(f.filterHits)) return EXIT_FAILURE; }
        else if (a == "--sort-results") f.sortResults = atoi(v.c_str());
        else if (a == "--min-length") f.orfMin = atoi(v.c_str());
        else if (a == "--max-length") f.orfMax = atoi(v.c_str());
        else if (a == "--max-gaps") f.orfGaps = atoi(v.c_str());
        else if (a == "--contig-start-mode") f.contigStart = atoi(v.c_str());
        else if (a == "--contig-end-mode") f.contigEnd = atoi(v.c_str());
        else if (a == "--orf-start-mode") f.orfStart = atoi(v.c_str());
        else if (a == "--forward-frames" || a == "--reverse-frames") {
            bool ok; const int m = frameMask(v, ok);
            if (!ok) { fprintf(stdout, "Error in argument %s\n", a.c_str()); return EXIT_FAILURE; }
            (a == "--forward-frames" ? f.fwdFrames : f.revFrames) = m;
        }
        else if (a == "--translation-table") f.translationTable = atoi(v.c_str());
        else if (a == "--translate") f.translate = atoi(v.c_str());
        else if (a == "--use-all-table-starts") { if (!setBool(f.allStarts)) return EXIT_FAILURE; }
        else if (a == "--add-orf-stop") { if (!setBool(f.addOrfStop)) return EXIT_FAILURE; }
        else if (a == "--preserve-keys") { if (!setBool(f.preserveKeys)) return EXIT_FAILURE; }
        else if (a == "--take-larger-entry") { if (!setBool(f.takeLarger)) return EXIT_FAILURE; }
        else if (a == "--sub-mat") {
            // only the matrices the tables were captured from: blosum62.out (amino acids) and nucleotide.out
            std::string aa, nu;
            const bool okA = multiParam(v, "aa", aa), okN = multiParam(v, "nucl", nu);
            if ((okA && baseName(aa) != "blosum62.out" && v.find(':') != std::string::npos) || (okN && baseName(nu) != "nucleotide.out" && v.find(':') != std::string::npos) ||
                (v.find(':') == std::string::npos && baseName(v) != "blosum62.out" && baseName(v) != "nucleotide.out")) {
                return unsupported("plass-hip: --sub-mat %s is not supported (built for blosum62.out / nucleotide.out)\n", v.c_str());
            }
        }
        else if (a == "--single-end") f.singleEnd = atoi(v.c_str());
        else if (a == "--shuffle") { if (!setBool(f.shuffle)) return EXIT_FAILURE; }
        else if (a == "--dbtype") f.dbtypeArg = atoi(v.c_str());
        else if (a == "--createdb-mode") f.createdbMode = atoi(v.c_str());
        else if (a == "--write-lookup") f.writeLookup = atoi(v.c_str());
        else if (a == "--id-offset" && mod == "createdb-reads") f.idOffset = strtoull(v.c_str(), nullptr, 10);
        else if (a == "--spaced-kmer-mode" || a == "--mask" || a == "--mask-lower-case" || a == "--compressed" || a == "--create-lookup" || a == "--id-offset") {
            if (atoi(v.c_str()) != 0) return unsupported("%s %s is not supported by plass-hip\n", a.c_str(), v.c_str());
        }
        else if (a == "--adjust-kmer-len") { int x = 0; if (!setBool(x)) return EXIT_FAILURE; if (x) return unsupported("--adjust-kmer-len is not supported by plass-hip\n"); }
        else if (a == "--spaced-kmer-pattern") { if (!v.empty()) return unsupported("--spaced-kmer-pattern is not supported by plass-hip\n"); }
        // --threads, -v, --db-load-mode, --split-memory-limit: no influence on the result
    }
    if (f.wrapped || f.filterHits || f.sortResults) return unsupported("--wrapped-scoring/--filter-hits/--sort-results are not supported by plass-hip\n");
    if (mod == "kmermatcher") {
        // the module's own defaults for these two are "choose automatically" (k = 0: from the DB size, kmermatcher.cpp:607-613;
        // --kmer-per-seq 0): not reproduced — every workflow passes them
        if (f.k <= 0 || f.kps <= 0) return unsupported("plass-hip kmermatcher: -k and --kmer-per-seq must be given (the automatic choice of the reference is not implemented)\n");
        // the reference's module default is spaced k-mers and masking ON unless told otherwise; the workflows run with both off
        // (setLinearFilterDefault turns them off for kmermatcher itself)
    }
    if (mod == "rescorediagonal" && f.rescoreMode != 3)
        return unsupported("plass-hip rescorediagonal: --rescore-mode %d is not part of the GPU path (the assembly workflows use mode 3)\n", f.rescoreMode);
    // Requests that are valid for the reference and lie outside the GPU path are all refused HERE, before the dry-run exit and before anything is
    // read or written (data/nuclassemble.sh:41,145 calls `concatdbs ... --preserve-keys` whenever circular contigs exist; with exit
    // code 1 the wrapper ended the workflow instead of handing the call to the reference, and the dry run reported it as accepted)
    if (mod == "concatdbs") {
        if (f.takeLarger) return unsupported("plass-hip concatdbs: --take-larger-entry is not part of the GPU path\n");
        if (pos.size() == 3) {      // sequence DBs, or the header DBs of ORF DBs (dbtype 12: data/assemble.sh:75); a DB that is not there yet cannot be probed (dry run on names only)
            const std::string tp = pos[0] + ".dbtype"; FILE *ft = fopen(tp.c_str(), "rb"); unsigned ty = 0;
            if (ft) {
                const bool got = fread(&ty, 4, 1, ft) == 1; fclose(ft);
                const int dbtype = got ? (int) (ty & 0x3FFFFFFFu) : -1;
                if (got && dbtype != PLASSHIP_DBTYPE_AMINO_ACIDS && dbtype != PLASSHIP_DBTYPE_NUCLEOTIDES && dbtype != 12)
                    return unsupported("plass-hip concatdbs: database type %d is not part of the GPU path (sequence DBs and ORF header DBs only)\n", dbtype);
                if (got && dbtype == 12 && f.preserveKeys) return unsupported("plass-hip concatdbs: --preserve-keys on a header DB is not part of the GPU path\n");
            }
        }
    }
    if (mod == "proteinaln2nucl" && pos.size() == 6 && (pos[0] == pos[1]) != (pos[2] == pos[3])) { fprintf(stdout, "Either query database == target database for nucleotide and amino acid or != for both\n"); return EXIT_FAILURE; }
    if (mod == "proteinaln2nucl" && pos.size() == 6 && pos[0] != pos[1])
        return unsupported("plass-hip proteinaln2nucl: separate query and target DBs are not part of the GPU path (the assembly workflows use one DB)\n");
    // mergereads (and the chains started from FASTQ pairs): the inputs KSeqFactory reads without this path's parser (KSeqWrapper.cpp:160-195)
    // are refused by name here; what only the contents show (FASTA, multi-line records, quality bytes >= 128) comes back from the library as
    // PLASSHIP_ERR_UNSUPPORTED before anything is written
    const size_t nChainOut = mod == "guidedassemble-chain" ? 2 : 1;
    std::vector<std::string> fastqIn;
    if (mod == "createdb-reads") {
        if (pos.size() < 2) { fprintf(stdout, "createdb-reads <i:file1[.gz]> ... <i:fileN[.gz]> <o:sequenceDB>\n"); return EXIT_FAILURE; }
        if (f.createdbMode != 0) return unsupported("plass-hip createdb-reads: --createdb-mode %d (soft links) is left to the reference\n", f.createdbMode);
        if (f.writeLookup != 1) return unsupported("plass-hip createdb-reads: --write-lookup %d is left to the reference\n", f.writeLookup);
        if (f.dbtypeArg < 0 || f.dbtypeArg > 2) { fprintf(stdout, "Error in argument --dbtype\n"); return EXIT_FAILURE; }
        if (f.dbtypeArg == 1) return unsupported("plass-hip createdb-reads: --dbtype 1 (amino acids) is not an input of the assembly workflows; left to the reference\n");
        if (f.idOffset > 0xFFFFFFFEull) { fprintf(stdout, "Error in argument --id-offset\n"); return EXIT_FAILURE; }
        fastqIn.assign(pos.begin(), pos.end() - 1);
    } else if (chain && f.singleEnd) {      // every positional before the output(s) is an unpaired read file (data/assemble.sh:27-38: createdb in place of mergereads)
        if (pos.size() < nChainOut + 1) { fprintf(stdout, "%s: --single-end 1 needs at least one read file before the output\n", mod.c_str()); return EXIT_FAILURE; }
        fastqIn.assign(pos.begin(), pos.end() - nChainOut);
    } else if (mod == "mergereads") {
        if (pos.size() < 3 || (pos.size() - 1) % 2) { fprintf(stdout, "mergereads <i:fastqFile1[.gz]> <i:fastqFile2[.gz]> ... <o:sequenceDB>\n"); return EXIT_FAILURE; }
        fastqIn.assign(pos.begin(), pos.end() - 1);
    } else if (chain && pos.size() > nChainOut + 1) {
        if ((pos.size() - nChainOut) % 2) { fprintf(stdout, "%s: one DB or pairs of FASTQ files before the output\n", mod.c_str()); return EXIT_FAILURE; }
        fastqIn.assign(pos.begin(), pos.end() - nChainOut);
    }
    for (const std::string &q : fastqIn) {
        if (q == "stdin") return unsupported("plass-hip %s: reading stdin is left to the reference\n", mod.c_str());
        if (q.size() >= 4 && q.compare(q.size() - 4, 4, ".bz2") == 0) return unsupported("plass-hip %s: bzip2 input (%s) is left to the reference\n", mod.c_str(), q.c_str());
    }
    // --fasta-out: the workflows' tail on the device (data/assemble.sh:159-201, nuclassemble.sh:138-207).  With --filter-proteins 1 (plass
    // assemble's default) the tail selects from filternoncoding's output, a network with the reference's weights: not on this path.
    if (!f.fastaOut.empty()) {
        if (mod == "assemble-chain" && f.filterProteins != 0)
            return unsupported("plass-hip assemble-chain: --fasta-out selects from filternoncoding's output with --filter-proteins 1; filternoncoding is outside the GPU path (pass --filter-proteins 0)\n");
        if (mod == "nuclassemble-chain" && f.contigOutputMode != 0 && f.contigOutputMode != 1) { fprintf(stdout, "--contig-output-mode must be 0 or 1\n"); return EXIT_FAILURE; }
        struct stat stF;
        if (stat(f.fastaOut.c_str(), &stF) == 0) { fprintf(stdout, "%s exists already!\n", f.fastaOut.c_str()); return EXIT_FAILURE; }     // data/assemble.sh:23, nuclassemble.sh:69
    }
    // --db-mode 1 --db-out DB (nuclassemble-chain) and --nuclassembly-out DB (guidedassemble-chain): the same tail ending in createsubdb's DB
    // instead of the FASTA file (nuclassemble.sh:200-207; the guided workflow runs its nuclassemble with --db-mode 1, GuidedNuclassembler.cpp:173)
    if (mod == "nuclassemble-chain" && (f.dbMode || !f.dbOut.empty())) {
        if (f.dbMode && !f.fastaOut.empty()) { fprintf(stdout, "nuclassemble-chain: --db-mode 1 writes a DB (--db-out), not a FASTA file: --fasta-out cannot be combined with it\n"); return EXIT_FAILURE; }
        if (!f.dbMode || f.dbOut.empty()) { fprintf(stdout, "nuclassemble-chain: --db-mode 1 and --db-out DB go together\n"); return EXIT_FAILURE; }
    }
    for (const std::string *o : {&f.dbOut, &f.nuclAssemblyOut}) {
        if (o->empty()) continue;
        if (f.contigOutputMode != 0 && f.contigOutputMode != 1) { fprintf(stdout, "--contig-output-mode must be 0 or 1\n"); return EXIT_FAILURE; }
        struct stat stO;
        if (stat(o->c_str(), &stO) == 0) { fprintf(stdout, "%s exists already!\n", o->c_str()); return EXIT_FAILURE; }     // nuclassemble.sh:69, guidedNuclAssemble.sh:24
    }
    if (!f.nuclAssemblyOut.empty() && f.numIterationsNucl < 1) { fprintf(stdout, "--num-iterations must be at least 1 (nucl)\n"); return EXIT_FAILURE; }
    // --resume 1 (assemble-chain, nuclassemble-chain): go on behind the highest complete DIR/assembly_<j> of an earlier run with the same
    // --write-intermediate DIR.  What cannot be right is refused here, before anything is read: a continuation with other parameters or
    // another input than DIR/chain.manifest records would be a chimera of two runs.
    int resumeFrom = -1; Manifest manifest;
    if (f.resume) {
        if (mod == "guidedassemble-chain") {
            // --write-intermediate keeps assembly_nucl_<i> only; the protein twins guidedassembleresults extends next to it (guidedassembleresult.cpp:340-365) are not stored
            fprintf(stdout, "guidedassemble-chain: --resume is not supported: --write-intermediate stores the nucleotide assembly without its protein twins, which is not enough to restart\n");
            return EXIT_FAILURE;
        }
        if (f.writeIntermediate.empty()) { fprintf(stdout, "%s: --resume 1 needs --write-intermediate DIR (the resume points are DIR/assembly_<i>)\n", mod.c_str()); return EXIT_FAILURE; }
        std::vector<std::string> inputs = fastqIn;
        if (inputs.empty() && !pos.empty()) for (const char *sfx : {"", ".index", ".dbtype"}) inputs.push_back(pos[0] + sfx);
        manifest = chainManifest(mod, f, inputs);
        resumeFrom = resumePoint(f.writeIntermediate, "assembly_", f.numIterations);
        if (resumeFrom >= 0) {
            const std::string mp = f.writeIntermediate + "/chain.manifest";
            if (!isFile(mp)) {
                fprintf(stdout, "%s: --resume 1: %s/assembly_%d.done exists but %s does not: what the stored DBs were computed with is unknown (delete the .done files to start over)\n",
                        mod.c_str(), f.writeIntermediate.c_str(), resumeFrom, mp.c_str());
                return EXIT_FAILURE;
            }
            std::string inFile; const std::string key = manifestDiffers(mp, manifest, inFile);
            if (!key.empty()) {
                std::string now; for (const auto &kv : manifest) if (kv.first == key) now = kv.second;
                fprintf(stdout, "%s: --resume 1: %s differs from the run that wrote %s/assembly_%d (%s: %s, this run: %s); delete the .done files to start over\n",
                        mod.c_str(), key.c_str(), f.writeIntermediate.c_str(), resumeFrom, mp.c_str(), inFile.c_str(), now.c_str());
                return EXIT_FAILURE;
            }
        }
    }
    if (getenv("PLASSHIP_CLI_DRYRUN") && atoi(getenv("PLASSHIP_CLI_DRYRUN")) != 0) {
        fprintf(stdout, "plass-hip dry run: %s accepted (%zu positional arguments, %zu flags); nothing read or computed\n", mod.c_str(), pos.size(), f.seen.size());
        return EXIT_DRYRUN_ACCEPTED;
    }
    plasship_ctx *ctx = nullptr;
    if (K(plasship_ctx_create(-1, &ctx))) return fail("plass-hip");
    const double t0 = now();
    int rc = EXIT_SUCCESS;
    if (mod == "kmermatcher") {
        if (pos.size() != 2) { fprintf(stdout, "kmermatcher <i:sequenceDB> <o:prefDB>\n"); return EXIT_FAILURE; }
        plasship_seqdb *db = nullptr; plasship_cands *c = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &db))) return fail("kmermatcher");
        int dbtype = 0; plasship_seqdb_info(db, nullptr, nullptr, nullptr, &dbtype, nullptr);
        plasship_kmermatch_params p; memset(&p, 0, sizeof(p));
        p.kmer_size = f.k; p.alphabet_size = f.alph; p.kmers_per_seq = f.kps; p.kmers_per_seq_scale = (dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES) ? f.scaleNucl : f.scaleAA;
        p.hash_shift = f.hashShift; p.include_only_extendable = f.onlyExt; p.ignore_multi_kmer = f.ignoreMulti; p.cov_mode = f.covMode; p.cov_thr = f.covThr;
        plasship_kmermatch_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_kmermatch(ctx, db, &p, &c, &st))) return fail("kmermatcher");
        fprintf(stdout, "k-mer records: %llu grouped: %llu candidates: %llu | kernels ms: extract %.3f partition %.3f group %.3f sort %.3f reduce %.3f\n",
                (unsigned long long) st.n_kmer_records, (unsigned long long) st.n_grouped, (unsigned long long) st.n_candidates,
                st.ms_extract, st.ms_sort1, st.ms_group, st.ms_sort2, st.ms_reduce);
        if (KW(plasship_cands_write(ctx, c, db, pos[1].c_str()))) return fail("kmermatcher");
        plasship_cands_free(ctx, c); plasship_seqdb_free(ctx, db);
    } else if (mod == "rescorediagonal") {
        if (pos.size() != 4) { fprintf(stdout, "rescorediagonal <i:queryDB> <i:targetDB> <i:prefDB> <o:alnDB>\n"); return EXIT_FAILURE; }
        plasship_seqdb *q = nullptr, *t = nullptr; plasship_cands *c = nullptr; plasship_alns *al = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &q))) return fail("rescorediagonal");
        if (pos[1] == pos[0]) t = q; else if (K(plasship_seqdb_read(ctx, pos[1].c_str(), &t))) return fail("rescorediagonal");
        if (K(plasship_cands_read(ctx, q, t, pos[2].c_str(), &c))) return fail("rescorediagonal");
        plasship_rescore_params p; memset(&p, 0, sizeof(p));
        p.rescore_mode = f.rescoreMode; p.eval_thr = f.evalThr; p.seq_id_thr = f.seqIdThr; p.cov_mode = f.covMode; p.cov_thr = f.covThr;
        p.min_aln_len = f.minAlnLen; p.seq_id_mode = f.seqIdMode; p.add_backtrace = f.addBt; p.include_identity = f.addSelf;
        plasship_rescore_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_rescore(ctx, q, t, c, &p, &al, &st))) return fail("rescorediagonal");
        fprintf(stdout, "scored: %llu accepted: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_scored, (unsigned long long) st.n_accepted, st.ms_kernel);
        if (KW(plasship_alns_write(ctx, al, pos[3].c_str()))) return fail("rescorediagonal");
        plasship_alns_free(ctx, al); plasship_cands_free(ctx, c); if (t != q) plasship_seqdb_free(ctx, t); plasship_seqdb_free(ctx, q);
    } else if (mod == "assembleresults" || mod == "nuclassembleresults") {
        if (pos.size() != 3) { fprintf(stdout, "%s <i:sequenceDB> <i:alnResult> <o:reprSeqDB>\n", mod.c_str()); return EXIT_FAILURE; }
        plasship_seqdb *db = nullptr, *o = nullptr; plasship_alns *al = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &db))) return fail("assembleresults");
        // the library picks the variant from the DB type (protein -> assembleresults, nucleotide -> nuclassembleresults);
        // the module name has to agree, the reference's assembleresults on nucleotides uses another comparator
        int dbtype = -1; plasship_seqdb_info(db, nullptr, nullptr, nullptr, &dbtype, nullptr);
        if ((mod == "nuclassembleresults") != (dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES)) {
            fprintf(stdout, "plass-hip: %s needs a %s sequence DB\n", mod.c_str(), mod == "nuclassembleresults" ? "nucleotide" : "protein");
            return EXIT_FAILURE;
        }
        if (K(plasship_alns_read(ctx, db, pos[1].c_str(), &al))) return fail("assembleresults");
        plasship_assemble_params p; memset(&p, 0, sizeof(p));
        p.seq_id_thr = f.seqIdThr; p.max_seq_len = f.maxSeqLen; p.keep_target = f.keepTarget; p.rescore_mode = f.rescoreMode;
        plasship_assemble_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_assemble(ctx, db, al, &p, &o, &st))) return fail("assembleresults");
        fprintf(stdout, "extended: %llu rescored: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_extended, (unsigned long long) st.n_rescored, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, o, pos[2].c_str()))) return fail("assembleresults");
        plasship_seqdb_free(ctx, o); plasship_alns_free(ctx, al); plasship_seqdb_free(ctx, db);
    } else if (mod == "guidedassembleresults") {
        if (pos.size() != 5) { fprintf(stdout, "guidedassembleresults <i:nuclSequenceDB> <i:aaSequenceDB> <i:nuclAlnResult> <o:nuclAssembly> <o:aaAssembly>\n"); return EXIT_FAILURE; }
        plasship_seqdb *nu = nullptr, *aa = nullptr, *on = nullptr, *oa = nullptr; plasship_alns *al = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &nu)) || K(plasship_seqdb_read(ctx, pos[1].c_str(), &aa))) return fail("guidedassembleresults");
        if (K(plasship_alns_read(ctx, nu, pos[2].c_str(), &al))) return fail("guidedassembleresults");
        plasship_assemble_params p; memset(&p, 0, sizeof(p));
        p.seq_id_thr = f.seqIdThr; p.max_seq_len = f.maxSeqLen; p.keep_target = f.keepTarget; p.rescore_mode = f.rescoreMode;
        plasship_assemble_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_guided_assemble(ctx, nu, aa, al, &p, &on, &oa, &st))) return fail("guidedassembleresults");
        fprintf(stdout, "extended: %llu rescored: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_extended, (unsigned long long) st.n_rescored, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, on, pos[3].c_str())) || KW(plasship_seqdb_write(ctx, oa, pos[4].c_str()))) return fail("guidedassembleresults");
        plasship_seqdb_free(ctx, on); plasship_seqdb_free(ctx, oa); plasship_alns_free(ctx, al); plasship_seqdb_free(ctx, aa); plasship_seqdb_free(ctx, nu);
    } else if (mod == "proteinaln2nucl") {
        if (pos.size() != 6) { fprintf(stdout, "proteinaln2nucl <i:queryNuclDB> <i:targetNuclDB> <i:queryAaDB> <i:targetAaDB> <i:alnDB> <o:alnDB>\n"); return EXIT_FAILURE; }
        plasship_seqdb *nu = nullptr, *aa = nullptr; plasship_alns *al = nullptr, *o = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &nu)) || K(plasship_seqdb_read(ctx, pos[2].c_str(), &aa))) return fail("proteinaln2nucl");
        if (K(plasship_alns_read(ctx, aa, pos[4].c_str(), &al))) return fail("proteinaln2nucl");
        plasship_aln2nucl_params p; p.gap_open = f.gapOpenNucl; p.gap_extend = f.gapExtendNucl;
        plasship_aln2nucl_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_aln2nucl(ctx, nu, nu, aa, aa, al, &p, &o, &st))) return fail("proteinaln2nucl");
        fprintf(stdout, "alignments: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_alignments, st.ms_kernel);
        if (KW(plasship_alns_write(ctx, o, pos[5].c_str()))) return fail("proteinaln2nucl");
        plasship_alns_free(ctx, o); plasship_alns_free(ctx, al); plasship_seqdb_free(ctx, aa); plasship_seqdb_free(ctx, nu);
    } else if (mod == "findassemblystart") {
        if (pos.size() != 3) { fprintf(stdout, "findassemblystart <i:sequenceDB> <i:alnDB> <o:sequenceDB>\n"); return EXIT_FAILURE; }
        plasship_seqdb *db = nullptr, *o = nullptr; plasship_alns *al = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &db))) return fail("findassemblystart");
        if (K(plasship_alns_read(ctx, db, pos[1].c_str(), &al))) return fail("findassemblystart");
        plasship_findstart_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_find_assembly_start(ctx, db, al, &o, &st))) return fail("findassemblystart");
        fprintf(stdout, "alignments: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_alignments, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, o, pos[2].c_str()))) return fail("findassemblystart");
        plasship_seqdb_free(ctx, o); plasship_alns_free(ctx, al); plasship_seqdb_free(ctx, db);
    } else if (mod == "cyclecheck") {
        if (pos.size() != 2) { fprintf(stdout, "cyclecheck <i:sequenceDB> <o:sequenceDBcycle>\n"); return EXIT_FAILURE; }
        plasship_seqdb *db = nullptr, *o = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &db))) return fail("cyclecheck");
        plasship_cyclecheck_params p; p.max_seq_len = f.maxSeqLen; p.chop_cycle = f.chopCycle;
        plasship_cyclecheck_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_cyclecheck(ctx, db, &p, &o, nullptr, &st))) return fail("cyclecheck");
        fprintf(stdout, "circular: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_cyclic, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, o, pos[1].c_str()))) return fail("cyclecheck");
        plasship_seqdb_free(ctx, o); plasship_seqdb_free(ctx, db);
    } else if (mod == "extractorfs") {
        // writes <out> and <out>_h like the reference (extractorfs.cpp:28-32)
        if (pos.size() != 2) { fprintf(stdout, "extractorfs <i:sequenceDB> <o:sequenceDB>\n"); return EXIT_FAILURE; }
        plasship_seqdb *db = nullptr, *o = nullptr; plasship_orfhdr *h = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &db))) return fail("extractorfs");
        plasship_orf_params p; memset(&p, 0, sizeof(p));
        p.min_length = f.orfMin; p.max_length = f.orfMax; p.max_gaps = f.orfGaps; p.contig_start_mode = f.contigStart; p.contig_end_mode = f.contigEnd;
        p.orf_start_mode = f.orfStart; p.forward_frames = f.fwdFrames; p.reverse_frames = f.revFrames; p.translation_table = f.translationTable;
        p.translate = f.translate; p.use_all_table_starts = f.allStarts; p.max_seq_len = f.maxSeqLen;
        plasship_orf_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_extract_orfs(ctx, db, &p, &o, &h, &st))) return fail("extractorfs");
        fprintf(stdout, "orfs: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_out, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, o, pos[1].c_str())) || KW(plasship_orfhdr_write(ctx, h, (pos[1] + "_h").c_str()))) return fail("extractorfs");
        plasship_orfhdr_free(ctx, h); plasship_seqdb_free(ctx, o); plasship_seqdb_free(ctx, db);
    } else if (mod == "translatenucs") {
        if (pos.size() != 2) { fprintf(stdout, "translatenucs <i:sequenceDB> <o:sequenceDB>\n"); return EXIT_FAILURE; }
        plasship_seqdb *db = nullptr, *o = nullptr; plasship_orfhdr *h = nullptr;
        if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &db))) return fail("translatenucs");
        if (f.addOrfStop && K(plasship_orfhdr_read(ctx, (pos[0] + "_h").c_str(), &h))) return fail("translatenucs");      // translatenucs.cpp:29-34
        plasship_translate_params p; p.translation_table = f.translationTable; p.add_orf_stop = f.addOrfStop; p.max_seq_len = f.maxSeqLen;
        plasship_orf_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_translate_nucs(ctx, db, h, &p, &o, &st))) return fail("translatenucs");
        fprintf(stdout, "translated: %llu | kernel ms: %.3f\n", (unsigned long long) st.n_out, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, o, pos[1].c_str()))) return fail("translatenucs");
        plasship_orfhdr_free(ctx, h); plasship_seqdb_free(ctx, o); plasship_seqdb_free(ctx, db);
    } else if (mod == "concatdbs") {
        if (pos.size() != 3) { fprintf(stdout, "concatdbs <i:DB> <i:DB> <o:DB>\n"); return EXIT_FAILURE; }
        // sequence DBs, or the header DBs of ORF DBs (dbtype 12: data/assemble.sh:75)
        int dbtype = -1;
        { std::string tp = pos[0] + ".dbtype"; FILE *ft = fopen(tp.c_str(), "rb"); unsigned ty = 0; if (ft && fread(&ty, 4, 1, ft) == 1) dbtype = (int) (ty & 0x3FFFFFFFu); if (ft) fclose(ft); }
        if (dbtype == PLASSHIP_DBTYPE_AMINO_ACIDS || dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES) {
            plasship_seqdb *a = nullptr, *b = nullptr, *o = nullptr;
            if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &a)) || K(plasship_seqdb_read(ctx, pos[1].c_str(), &b))) return fail("concatdbs");
            if (K(plasship_seqdb_concat_keys(ctx, a, b, f.preserveKeys, &o))) return fail("concatdbs");
            if (KW(plasship_seqdb_write(ctx, o, pos[2].c_str()))) return fail("concatdbs");
            plasship_seqdb_free(ctx, o); plasship_seqdb_free(ctx, b); plasship_seqdb_free(ctx, a);
        } else if (dbtype == 12) {
            plasship_orfhdr *a = nullptr, *b = nullptr, *o = nullptr;
            if (K(plasship_orfhdr_read(ctx, pos[0].c_str(), &a)) || K(plasship_orfhdr_read(ctx, pos[1].c_str(), &b))) return fail("concatdbs");
            if (K(plasship_orfhdr_concat(ctx, a, b, &o))) return fail("concatdbs");
            if (KW(plasship_orfhdr_write(ctx, o, pos[2].c_str()))) return fail("concatdbs");
            plasship_orfhdr_free(ctx, o); plasship_orfhdr_free(ctx, b); plasship_orfhdr_free(ctx, a);
        } else { fprintf(stdout, "plass-hip concatdbs: cannot read the database type of %s\n", pos[0].c_str()); return EXIT_FAILURE; }      // (other types were refused above)
    } else if (mod == "createdb-reads") {
        // writes <out>, <out>_h, <out>.lookup and <out>.source like the reference's createdb (createdb.cpp:84,92-95,291-329)
        std::vector<const char *> files; for (const std::string &q : fastqIn) files.push_back(q.c_str());
        plasship_createdb_params cp; cp.shuffle = f.shuffle; cp.id_offset = (uint32_t) f.idOffset; cp.dbtype = f.dbtypeArg;
        plasship_createdb_stats st; memset(&st, 0, sizeof(st));
        if (KW(plasship_createdb_write(ctx, files.data(), files.size(), &cp, pos.back().c_str(), nullptr, &st))) return fail("createdb-reads");
        fprintf(stdout, "entries: %llu lines: %llu chunks: %llu | read %.3f s upload %.3f s kernels %.3f ms (write %.3f ms) total %.3f s\n", (unsigned long long) st.entries,
                (unsigned long long) st.lines, (unsigned long long) st.chunks, st.ms_read * 1e-3, st.ms_upload * 1e-3, st.ms_kernel, st.ms_write_kernel, st.ms_total * 1e-3);
    } else if (mod == "mergereads") {
        // writes <out> and <out>_h like the reference (mergereads.cpp:28-31)
        std::vector<const char *> files; for (const std::string &q : fastqIn) files.push_back(q.c_str());
        plasship_seqdb *r = nullptr, *h = nullptr;
        plasship_merge_stats st; memset(&st, 0, sizeof(st));
        if (K(plasship_mergereads(ctx, files.data(), files.size(), nullptr, &r, &h, &st))) return fail("mergereads");
        fprintf(stdout, "pairs: %llu combined: %llu not combined: %llu | parse %.3f s upload %.3f s kernels %.3f ms\n", (unsigned long long) st.pairs,
                (unsigned long long) st.combined, (unsigned long long) st.not_combined, st.ms_parse * 1e-3, st.ms_upload * 1e-3, st.ms_kernel);
        if (KW(plasship_seqdb_write(ctx, r, pos.back().c_str())) || KW(plasship_seqdb_write(ctx, h, (pos.back() + "_h").c_str()))) return fail("mergereads");
        plasship_seqdb_free(ctx, h); plasship_seqdb_free(ctx, r);
    } else if (chain) {
        // ---- fused drivers: the iteration loop of a workflow script with every DB of the loop resident in HBM; only the first DB is
        //      read from disk and only the last one written (plus, with --write-intermediate DIR, every iteration's assembly by a host
        //      thread on a second context while the next iteration runs, with the workflow's .done sentinels) ----
        const bool prot = mod == "assemble-chain", nuc = mod == "nuclassemble-chain", gd = mod == "guidedassemble-chain";
        if (pos.size() != (gd ? 3u : 2u) && fastqIn.empty()) { fprintf(stdout, "%s: wrong number of databases\n", mod.c_str()); return EXIT_FAILURE; }
        const std::vector<std::string> outs(pos.end() - nChainOut, pos.end());
        if (f.numIterations < 1) { fprintf(stdout, "--num-iterations must be at least 1\n"); return EXIT_FAILURE; }
        plasship_ctx *wctx = nullptr; std::thread writer; int writerRc = 0; std::string writerErr;
        // every exit path below joins the writer first (a joinable std::thread that goes out of scope terminates the process, and an
        // intermediate DB must not be left half written behind an ordinary error message: ADVICE r3)
        struct JoinOnExit { std::thread &t; ~JoinOnExit() { if (t.joinable()) t.join(); } } joinOnExit{writer};
        if (!f.writeIntermediate.empty() && K(plasship_ctx_create(-1, &wctx))) return fail(mod.c_str());
        auto joinWriter = [&]() { if (writer.joinable()) writer.join(); return writerRc; };
        auto writeAsync = [&](const plasship_seqdb *d, const std::string &name) {
            if (!wctx) return;
            joinWriter();
            const std::string path = f.writeIntermediate + "/" + name;
            writer = std::thread([&, d, path]() {
                if (plasship_seqdb_write(wctx, d, path.c_str())) { writerRc = 1; writerErr = plasship_last_error(); return; }      // (the error text is the writer THREAD's)
                FILE *fd = fopen((path + ".done").c_str(), "w"); if (fd) fclose(fd); else writerRc = 1;     // data/assemble.sh:147 `touch assembly_$STEP.done`
            });
        };
        // a tail (--fasta-out; --db-mode 1 --db-out; --nuclassembly-out) needs SOURCE — the DB the loop starts from — and, on nucleotides,
        // every iteration's circular contigs: the loop keeps both
        const bool wantFasta = !f.fastaOut.empty(), wantDb = nuc && f.dbMode, wantNuclAsm = gd && !f.nuclAssemblyOut.empty();
        if (f.resume && resumeFrom < 0 && !writeManifest(f.writeIntermediate + "/chain.manifest", manifest)) {
            fprintf(stdout, "%s: cannot write %s/chain.manifest\n", mod.c_str(), f.writeIntermediate.c_str()); return EXIT_FAILURE;
        }
        // a resumed run reads DIR/assembly_<j> in place of the input; only a tail still needs the input, as SOURCE, made the way a fresh run makes it
        plasship_seqdb *in = nullptr, *db = nullptr, *aa = nullptr; double tRead = now();
        if (resumeFrom < 0 || wantFasta || wantDb) {
            // a multi-GB input: the library takes its device arena (seconds of hipMalloc) while this thread reads and parses the DB files
            { struct stat stIn; if (stat(pos[0].c_str(), &stIn) == 0 && stIn.st_size >= ((off_t) 1 << 30)) (void) plasship_ctx_reserve_async(ctx); }
            if (!fastqIn.empty() && f.singleEnd) {      // the workflows' createdb step for unpaired input (data/assemble.sh:27-38): the reads stay in HBM
                std::vector<const char *> files; for (const std::string &q : fastqIn) files.push_back(q.c_str());
                plasship_createdb_stats cs;
                if (K(plasship_createdb(ctx, files.data(), files.size(), nullptr, &in, &cs))) return fail(mod.c_str());
                fprintf(stdout, "createdb: %llu reads from %llu files\n", (unsigned long long) cs.entries, (unsigned long long) cs.files);
            } else if (!fastqIn.empty()) {         // the workflows' mergereads step (data/assemble.sh:27-38): the merged reads stay in HBM, the header DB is not needed
                std::vector<const char *> files; for (const std::string &q : fastqIn) files.push_back(q.c_str());
                plasship_seqdb *h = nullptr; plasship_merge_stats ms;
                if (K(plasship_mergereads(ctx, files.data(), files.size(), nullptr, &in, &h, &ms))) return fail(mod.c_str());
                plasship_seqdb_free(ctx, h);
                fprintf(stdout, "mergereads: %llu pairs, %llu combined\n", (unsigned long long) ms.pairs, (unsigned long long) ms.combined);
            } else if (K(plasship_seqdb_read(ctx, pos[0].c_str(), &in))) return fail(mod.c_str());
            tRead = now();
            int dbtype = -1; plasship_seqdb_info(in, nullptr, nullptr, nullptr, &dbtype, nullptr);
            auto orfPar = [&](bool start) {       // the two extractorfs passes (Assembler.cpp:116-130, GuidedNuclassembler.cpp:133-145)
                plasship_orf_params p; memset(&p, 0, sizeof(p));
                p.min_length = start ? 20 : 45; p.max_length = start ? 45 : 32734; p.max_gaps = 0; p.contig_start_mode = start ? 1 : 2; p.contig_end_mode = start ? 0 : 2;
                p.orf_start_mode = 0; p.forward_frames = 7; p.reverse_frames = 7; p.translation_table = 1; p.max_seq_len = 65535;
                return p;
            };
            plasship_translate_params tp; tp.translation_table = 1; tp.add_orf_stop = 1; tp.max_seq_len = 65535;
            db = in;          // protein / nucleotide chain: db; guided chain: db = nucleotide ORFs, aa = their twins
            if (gd || (prot && (f.fromReads || dbtype == PLASSHIP_DBTYPE_NUCLEOTIDES))) {
                if (dbtype != PLASSHIP_DBTYPE_NUCLEOTIDES) { fprintf(stdout, "%s: the input must be a nucleotide read DB\n", mod.c_str()); return EXIT_FAILURE; }
                plasship_seqdb *ol = nullptr, *os = nullptr; plasship_orfhdr *hl = nullptr, *hs = nullptr; plasship_orf_stats ost;
                const plasship_orf_params pl = orfPar(false), ps = orfPar(true);
                if (K(plasship_extract_orfs(ctx, in, &pl, &ol, &hl, &ost)) || K(plasship_extract_orfs(ctx, in, &ps, &os, &hs, &ost))) return fail(mod.c_str());
                if (gd) {      // concatdbs of ORFs and headers, then one translatenucs (data/guidedNuclAssemble.sh:56-75)
                    plasship_seqdb *nu = nullptr; plasship_orfhdr *hh = nullptr;
                    if (K(plasship_seqdb_concat(ctx, ol, os, &nu)) || K(plasship_orfhdr_concat(ctx, hl, hs, &hh)) || K(plasship_translate_nucs(ctx, nu, hh, &tp, &aa, &ost))) return fail(mod.c_str());
                    plasship_orfhdr_free(ctx, hh); db = nu;
                } else {       // translatenucs x2, then concatdbs (data/assemble.sh:41-77)
                    plasship_seqdb *al = nullptr, *as = nullptr;
                    if (K(plasship_translate_nucs(ctx, ol, hl, &tp, &al, &ost)) || K(plasship_translate_nucs(ctx, os, hs, &tp, &as, &ost)) || K(plasship_seqdb_concat(ctx, al, as, &db))) return fail(mod.c_str());
                    plasship_seqdb_free(ctx, al); plasship_seqdb_free(ctx, as);
                }
                plasship_orfhdr_free(ctx, hl); plasship_orfhdr_free(ctx, hs); plasship_seqdb_free(ctx, ol); plasship_seqdb_free(ctx, os);
                if (!(gd && !f.nuclAssemblyOut.empty())) { plasship_seqdb_free(ctx, in); in = nullptr; }      // (the guided tail concatenates the reads: guidedNuclAssemble.sh:161-165)
            } else if ((prot && dbtype != PLASSHIP_DBTYPE_AMINO_ACIDS) || (nuc && dbtype != PLASSHIP_DBTYPE_NUCLEOTIDES)) {
                fprintf(stdout, "%s: wrong input DB type %d\n", mod.c_str(), dbtype); return EXIT_FAILURE;
            }
        }
        const double tPrep = now();
        ChainLoop L;
        L.ctx = ctx; L.name = mod.c_str(); L.kind = prot ? CHAIN_PROTEIN : nuc ? CHAIN_NUCL : CHAIN_GUIDED;
        L.numIterations = f.numIterations; L.k = f.k; L.alph = f.alph; L.kps = f.kps; L.kpsScale = nuc ? f.scaleNucl : f.scaleAA; L.ignoreMulti = f.ignoreMulti;
        L.covMode = f.covMode; L.covThr = f.covThr; L.hashShift = f.hashShift; L.gapOpenNucl = f.gapOpenNucl; L.gapExtendNucl = f.gapExtendNucl;
        L.chopCycle = f.chopCycle; L.maxSeqLen = f.maxSeqLen;
        memset(&L.rp, 0, sizeof(L.rp));
        L.rp.rescore_mode = f.rescoreMode; L.rp.eval_thr = f.evalThr; L.rp.seq_id_thr = f.seqIdThr; L.rp.cov_mode = f.covMode; L.rp.cov_thr = f.covThr; L.rp.min_aln_len = f.minAlnLen;
        L.rp.seq_id_mode = f.seqIdMode; L.rp.add_backtrace = gd ? 1 : 0;
        memset(&L.ap, 0, sizeof(L.ap));
        L.ap.seq_id_thr = gd ? f.seqIdThrNucl : f.seqIdThr; L.ap.max_seq_len = f.maxSeqLen; L.ap.keep_target = f.keepTarget; L.ap.rescore_mode = f.rescoreMode;
        L.keepForTail = wantFasta || wantDb || wantNuclAsm;
        if (nuc) L.cyclePrefix = outs[0] + "_cycle_";
        L.intermediateName = gd ? "assembly_nucl_" : "assembly_";
        L.joinWriter = [&]() { if (joinWriter()) { fprintf(stdout, "%s: writing an intermediate DB failed: %s\n", mod.c_str(), writerErr.c_str()); return 1; } return 0; };
        L.writeAsync = writeAsync;
        L.writeLastIntermediate = f.resume != 0;
        if (resumeFrom >= 0) {
            // DIR/assembly_<j> is the DB iteration j handed to iteration j + 1: on nucleotides the rest after cyclecheck took the circular contigs out
            // (they are in <o>_cycle_<i>).  The library's caches (selected windows, positions, cyclecheck's "rest" lineage) start cold, as they do
            // for any DB read from files; none of them changes a result.
            const std::string from = f.writeIntermediate + "/" + L.intermediateName + std::to_string(resumeFrom);
            fprintf(stdout, "resuming at iteration %d (from %s)\n", resumeFrom + 1, from.c_str());
            L.startIteration = resumeFrom + 1; L.source = db; db = nullptr;
            if (K(plasship_seqdb_read(ctx, from.c_str(), &db))) return fail(mod.c_str());
            int dbtypeFrom = -1; plasship_seqdb_info(db, nullptr, nullptr, nullptr, &dbtypeFrom, nullptr);
            if (dbtypeFrom != (prot ? PLASSHIP_DBTYPE_AMINO_ACIDS : PLASSHIP_DBTYPE_NUCLEOTIDES)) { fprintf(stdout, "%s: wrong DB type %d of %s\n", mod.c_str(), dbtypeFrom, from.c_str()); return EXIT_FAILURE; }
            // PREV_CYCLE_ALL of the tail: the circular contigs of the iterations up to j, from the files the interrupted run wrote next to its output
            for (int i = 0; nuc && L.keepForTail && i <= resumeFrom; i++) {
                const std::string cp = L.cyclePrefix + std::to_string(i);
                if (!isFile(cp) || !isFile(cp + ".index")) continue;       // (an iteration without circular contigs writes no file)
                plasship_seqdb *cyc = nullptr;
                if (K(plasship_seqdb_read(ctx, cp.c_str(), &cyc))) return fail(mod.c_str());
                if (!L.cycAll) { L.cycAll = cyc; continue; }
                plasship_seqdb *u = nullptr;
                if (K(plasship_seqdb_concat_keys(ctx, L.cycAll, cyc, 1, &u))) return fail(mod.c_str());
                plasship_seqdb_free(ctx, L.cycAll); plasship_seqdb_free(ctx, cyc); L.cycAll = u;
            }
        }
        L.db = db; L.aa = aa; L.tStart = tPrep;
        if (const int rcL = runChainLoop(L)) return rcL;
        db = L.db; aa = L.aa;
        const double tLoop = now();
        if (L.joinWriter()) return EXIT_FAILURE;
        if (KW(plasship_seqdb_write(ctx, db, outs[0].c_str())) || (gd && KW(plasship_seqdb_write(ctx, aa, outs[1].c_str())))) return fail(mod.c_str());
        if (wantFasta || wantDb) {
            if (const int rcT = chainTail(ctx, mod.c_str(), nuc, db, L.source, L.cycAll, f.contigOutputMode, f.minContigLen, f.fastaOut, f.dbOut)) return rcT;
        }
        double tTail = 0;
        if (wantNuclAsm) {
            // ---- data/guidedNuclAssemble.sh:135-170 on the handles of the loop above ----
            const double tt0 = now();
            // `_only_assembled` (guidedNuclAssemble.sh:136-139): the entries of the last assembly_nucl_<i> whose key nucl_6f_start_long holds with a
            // shorter entry, `$3 > $6`; no length threshold — the nucleotide selection with only_extended and --min-contig-len 0 (include/plasship.h)
            plasship_select_params sp; memset(&sp, 0, sizeof(sp));
            sp.mode = PLASSHIP_SELECT_NUCLEOTIDE; sp.only_extended = 1; sp.min_contig_len = 0;
            plasship_seqdb *only = nullptr, *mergedIn = nullptr; plasship_select_stats ss;
            if (K(plasship_select_contigs(ctx, db, L.source, nullptr, &sp, &only, &ss))) return fail(mod.c_str());
            // concatdbs <only_assembled> <reads> guided_assembly.merged (guidedNuclAssemble.sh:161-165): the subset's keys are kept, the reads follow
            // from max(key) + 1 on in the order of their data file (DBConcat.cpp:63-118; 1 when nothing was selected: DBConcat.cpp:63,100)
            if (K(plasship_seqdb_concat(ctx, only, in, &mergedIn))) return fail(mod.c_str());
            size_t nAsm = 0, nMerged = 0; plasship_seqdb_info(db, &nAsm, nullptr, nullptr, nullptr, nullptr); plasship_seqdb_info(mergedIn, &nMerged, nullptr, nullptr, nullptr, nullptr);
            fprintf(stdout, "guided tail: %llu of %zu extended ORFs + the reads = %zu sequences\n", (unsigned long long) ss.n_selected, nAsm, nMerged);
            plasship_seqdb_free(ctx, only); plasship_seqdb_free(ctx, L.source); L.source = nullptr; plasship_seqdb_free(ctx, in); in = nullptr;
            // nuclassemble <merged> <out> --db-mode 1 (guidedNuclAssemble.sh:167-170): the nucleotide halves of the multi-parameters
            // (GuidedNuclassembler.cpp:167-172), everything else as penguin nuclassemble runs it (Nuclassembler.cpp:10-31)
            ChainLoop N;
            N.ctx = ctx; N.name = mod.c_str(); N.kind = CHAIN_NUCL;
            N.numIterations = f.numIterationsNucl; N.k = f.kNucl; N.alph = f.alph; N.kps = f.kps; N.kpsScale = f.scaleNucl; N.ignoreMulti = f.ignoreMulti;
            N.covMode = 0; N.covThr = f.covThr; N.hashShift = f.hashShift; N.chopCycle = f.chopCycle; N.maxSeqLen = f.maxSeqLen;
            memset(&N.rp, 0, sizeof(N.rp));
            N.rp.rescore_mode = f.rescoreMode; N.rp.eval_thr = f.evalThr; N.rp.seq_id_thr = f.seqIdThrNucl; N.rp.cov_mode = 0; N.rp.cov_thr = f.covThr; N.rp.min_aln_len = f.minAlnLenNucl;
            N.rp.seq_id_mode = f.seqIdMode; N.rp.add_backtrace = 0;
            N.ap = L.ap;
            N.keepForTail = true;
            N.db = mergedIn; N.tStart = tt0;
            if (const int rcN = runChainLoop(N)) return rcN;
            if (const int rcT = chainTail(ctx, mod.c_str(), true, N.db, N.source, N.cycAll, f.contigOutputMode, f.minContigLen, std::string(), f.nuclAssemblyOut)) return rcT;
            plasship_seqdb_free(ctx, N.db);
            L.overlaps += N.overlaps; L.kernelMs += N.kernelMs;
            tTail = now() - tt0;
        }
        const double tEnd = now();
        fprintf(stdout, "chain: %d iterations, %llu candidate overlaps | read %.3fs preprocessing %.3fs iterations %.3fs (kernels %.3fs) write %.3fs", f.numIterations, L.overlaps,
                tRead - t0, tPrep - tRead, tLoop - tPrep, L.kernelMs * 1e-3, tEnd - tLoop - tTail);
        if (wantNuclAsm) fprintf(stdout, " nuclassembly (%d iterations) %.3fs", f.numIterationsNucl, tTail);
        fprintf(stdout, "\n");
        plasship_seqdb_free(ctx, db); if (gd) plasship_seqdb_free(ctx, aa);
        if (wctx) plasship_ctx_destroy(wctx);
    }
    fprintf(stdout, "Time for processing: %.3fs\n", now() - t0);
    // Every output DB is complete and renamed into place by now.  Taking the context apart — unmapping an arena of up to 270 GB, the runtime's own
    // shutdown — is work the driver does for an exiting process anyway; a command-line tool leaves it to it (round 6: ~1 s of the fused driver's wall
    // clock at 50 M reads).  PLASSHIP_CLI_FULL_TEARDOWN=1: the orderly way (leak checkers).
    fflush(stdout); fflush(stderr);
    if (!getenv("PLASSHIP_CLI_FULL_TEARDOWN")) _exit(rc);
    plasship_ctx_destroy(ctx);
    return rc;
}
