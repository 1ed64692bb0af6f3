// GENERATION-TIME TOOL (build container only; never shipped, never run on the GPU box).
//
// Links the UNMODIFIED lib/flash of the reference (combine_reads.cpp, read.cpp, util.cpp; tests/golden/make_mergereads_ladder.sh compiles
// them) and does for every read pair of two FASTQ files what the reference's mergereads does with it (src/assembler/mergereads.cpp:19-24,
// 75-111): the same five combine_params, reverse_complement(r2), combine_reads(r1, r2, combined).  It prints, per pair, one line with the
// status (1 combined, 0 not) and then the one or two sequence entries the reference would write, one per line, so that the outcome can
// be committed as DATA.  The files are read here as strict four-line FASTQ, NOT through kseq: the parser's rules (CR LF, names, refusals)
// are pinned elsewhere.  This file contains no reference code; it only calls it.
//
//   flash_pin <reads_1.fastq> <reads_2.fastq>  >  expected
#include <flash/combine_reads.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

struct Rec { std::string seq, qual; };

static std::vector<Rec> readFastq(const char *path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { std::cerr << "flash_pin: cannot open " << path << "\n"; exit(1); }
    std::vector<Rec> out;
    std::string h, s, p, q;
    while (std::getline(in, h)) {
        if (!std::getline(in, s) || !std::getline(in, p) || !std::getline(in, q) || h.empty() || h[0] != '@' || p.empty() || p[0] != '+' ||
            s.empty() || s.size() != q.size()) { std::cerr << "flash_pin: " << path << ": not strict four-line FASTQ at record " << out.size() + 1 << "\n"; exit(1); }
        out.push_back({s, q});
    }
    return out;
}

static void line(const char *s, int n) { fwrite(s, 1, (size_t) n, stdout); fputc('\n', stdout); }

int main(int argc, char **argv) {
    if (argc != 3) { std::cerr << "usage: flash_pin <reads_1.fastq> <reads_2.fastq>\n"; return 2; }
    std::vector<Rec> f1 = readFastq(argv[1]), f2 = readFastq(argv[2]);
    combine_params par;
    par.max_overlap = 65;
    par.min_overlap = 15;
    par.max_mismatch_density = 0.10;
    par.cap_mismatch_quals = false;
    par.allow_outies = false;
    struct read *r1 = (struct read *) calloc(1, sizeof(struct read)), *r2 = (struct read *) calloc(1, sizeof(struct read));
    struct read *rc = (struct read *) calloc(1, sizeof(struct read));
    for (size_t k = 0; k < f1.size() && k < f2.size(); k++) {
        r1->seq = &f1[k].seq[0]; r1->seq_len = (int) f1[k].seq.size(); r1->qual = &f1[k].qual[0]; r1->qual_len = (int) f1[k].qual.size();
        r2->seq = &f2[k].seq[0]; r2->seq_len = (int) f2[k].seq.size(); r2->qual = &f2[k].qual[0]; r2->qual_len = (int) f2[k].qual.size();
        reverse_complement(r2);
        const enum combine_status st = combine_reads(r1, r2, rc, &par);
        if (st == NOT_COMBINED) { puts("0"); line(r1->seq, r1->seq_len); line(r2->seq, r2->seq_len); }
        else { puts("1"); line(rc->seq, rc->seq_len); }
    }
    return 0;
}
