// plasship: extractorfs and translatenucs with any genetic code the reference accepts (--translation-table, --use-all-table-starts).  Product code,
// built into the extension library libplasship_gencode.so (include/plasship_ext/gencode.h).  plasship_extract_orfs and plasship_translate_nucs keep
// their answers (the standard code with ATG, anything else refused); the entry points below take the same structs and handles and every table of
//   mm/commons/TranslateNucl.h:82-246   ids 1-6, 9-16, 21-31; another id ends the reference with "Invalid translation table selected!"
//   mm/commons/Orf.cpp:55-91            the scan's stop codons and, with useAllTableStarts, its start codons come from the table
// The kernels, the tables and the host code are those of orfs.hip in libplasship.so (orfKernel<PASS, true> reads the two codon sets as 64-bit masks;
// the translation LUT is built per table); this file is the library's exported surface.
#include "common.hpp"
#include "../../include/plasship_ext/gencode.h"

extern "C" int plasship_gencode_info(int table, char residues[65], char starts[65]) { return plasship::gencodeInfo(table, residues, starts); }

extern "C" int plasship_extract_orfs_gc(plasship_ctx *ctx, const plasship_seqdb *reads, const plasship_orf_params *par, plasship_seqdb **out_orfs,
                                        plasship_orfhdr **out_hdr, plasship_orf_stats *stats) {
    return plasship::extractOrfsGencode(ctx, reads, par, out_orfs, out_hdr, stats);
}

extern "C" int plasship_translate_nucs_gc(plasship_ctx *ctx, const plasship_seqdb *orfs, const plasship_orfhdr *hdr, const plasship_translate_params *par,
                                          plasship_seqdb **out_aa, plasship_orf_stats *stats) {
    return plasship::translateNucsGencode(ctx, orfs, hdr, par, out_aa, stats);
}
