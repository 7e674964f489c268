// fq_vcf.h -- the chunked reader of `svd`'s panel VCFs (fq_svd_read_panel; DESIGN 5v "the panel reader"): SVDcalculator::ReadVcf's per-line work, stated once for
// host and device.  fq_vcf.cpp drives it over chunks of text; fq_device.hip wraps the bodies below in kernels (reader 1), fq_vcf.cpp runs them as host loops
// (reader 2, the CPU tier).  The serial reader (fq_svd.cpp) stays the yardstick.
//
//   line ends          launch_nl_index (the FASTQ front end's)
//   fq_vcf_site_line   a thread per line: CHROM, POS, REF / first ALT lengths, acceptChr, the FORMAT key (PL before GL before GT) and its index, where column
//                      9 begins; under --Sites the site test.  One FqVcfLine per line.
//   compaction         launch_scan over the lines' keep words, fq_vcf_compact_line scatters the kept lines' numbers in input order
//   fq_vcf_cell        the genotype of ONE plain cell.  k_vcf_geno: a workgroup per kept line walks it in 4 KiB tiles -- 16 bytes a thread, the tabs marked, a prefix
//                      sum over the block's tab counts numbers the columns -- and the thread that owns a cell's first byte parses it.  The host loop walks the
//                      same line tab by tab and calls the same fq_vcf_cell.
// Whatever is not plain -- another cell form, the GL key (atof), a column count other than the header's, a value that leads to a refusal -- sets the line's
// needs_host, and the host's per-record statement (fq_svd_host.h: fq_svd_record) parses the line: its verdicts and messages stand.
// Bounds: every loop below ends at the line's end, which is at most n (the chunk's text is text[0, n)); no byte outside [text, text + n) is read.
#pragma once
#include "fq_common.h"
#include <cstdint>
#include <cstddef>

#define FQV_TILE 4096u          // bytes of a line a workgroup of k_vcf_geno takes at a time: 256 threads x 16 bytes
#define FQV_CELL_MAX 255u       // a cell longer than this is not plain
#define FQV_CHROM_INLINE 7u     // a CHROM this long travels in the line's record (chr22: 5); a longer one is never a kept marker's
#define FQV_NEEDS_HOST (-128)   // fq_vcf_cell: not a plain cell

enum {
  FQV_F_EMPTY = 1u << 0,        // an empty line (ends the file)
  FQV_F_LT5 = 1u << 1,          // fewer than 5 columns
  FQV_F_LT10 = 1u << 2,         // fewer than 10 columns
  FQV_F_HASH = 1u << 3,         // begins with '#'
  FQV_F_CHROM_OK = 1u << 4,     // acceptChr
  FQV_F_INDEL = 1u << 5,        // REF or the first ALT longer than one base
  FQV_F_NOALLELE = 1u << 6,     // REF or the first ALT empty
  FQV_F_NOKEY = 1u << 7,        // FORMAT has none of PL, GL, GT
  FQV_F_SITE = 1u << 8,         // passes the site test (set on every line when there are no sites)
  FQV_F_HOST = 1u << 9,         // the line goes to the host's statement as it is (a GL key, a POS of more than 18 digits, a key index beyond 255, ...)
  FQV_F_LONGCHROM = 1u << 10,   // CHROM longer than FQV_CHROM_INLINE
  FQV_F_GENO = 1u << 11,        // a kept line: k_vcf_geno parses its cells
};
enum { FQV_KEY_PL = 0, FQV_KEY_GL = 1, FQV_KEY_GT = 2 };

struct FqVcfLine {
  uint32_t beg, len;            // the line is text[beg, beg + len): no line end, no CR in front of it
  int32_t pos;                  // atoi(POS)
  uint32_t flags;
  uint32_t col9;                // where column 9 (the first genotype cell) begins, as a position in the text
  int32_t site;                 // the site's place in the sorted keys, or -1
  uint16_t n_keys;              // ':' fields of FORMAT
  uint8_t key_idx, key;         // the selected key's index and kind (FQV_KEY_*)
  uint8_t chrom_len;
  char chrom[FQV_CHROM_INLINE];
  char ref, alt;                // the first bytes of REF and ALT
  uint8_t pad[2];
};
// the sites: sorted keys (chromosome ordinal << 32 | position), the chromosomes' names ('chr' / 'CHR' removed) back to back
struct FqVcfSites {
  const uint64_t *keys; uint32_t n_keys;
  const char *names; const uint32_t *name_off; uint32_t n_names;      // name k is names[name_off[k], name_off[k + 1])
  uint8_t *found;               // [n_keys]: set to 1 where a record is handed to the reader
};
struct FqVcfSiteArgs {
  const uint8_t *text; uint32_t n, lo;        // lines of text[lo, n); nl[i] is the end of line i
  const uint32_t *nl; uint32_t n_lines;
  FqVcfLine *line; uint32_t *keep;            // keep[i]: 1 where k_vcf_geno parses line i
  FqVcfSites sites;                           // (n_keys == 0 and keys == nullptr: no site test)
  int32_t use_sites;
};
struct FqVcfGenoArgs {
  const uint8_t *text; uint32_t n;
  const FqVcfLine *line; const uint32_t *kept; uint32_t n_kept;   // kept[k]: the line of kept row k
  int32_t n_sample;
  int8_t *g;                    // [n_kept][n_sample]
  uint32_t *needs_host;         // [n_kept], zero on entry
};

FQ_HD bool fqv_is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
FQ_HD uint8_t fqv_upper(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }
FQ_HD bool fqv_is_acgt(uint8_t c) { c = fqv_upper(c); return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// the site test: (a) CHROM ('chr' / 'CHR' removed) and POS are a site's; (b) REF is one base and some ALT allele is one base of ACGTacgt other than REF
FQ_HD int32_t fqv_site_of(const FqVcfSites &S, const uint8_t *chrom, uint32_t clen, int32_t pos) {
  if (clen >= 3 && ((chrom[0] == 'c' && chrom[1] == 'h' && chrom[2] == 'r') || (chrom[0] == 'C' && chrom[1] == 'H' && chrom[2] == 'R'))) { chrom += 3; clen -= 3; }
  uint32_t ord = S.n_names;
  for (uint32_t k = 0; k < S.n_names && ord == S.n_names; ++k) {
    const uint32_t a = S.name_off[k], l = S.name_off[k + 1] - a;
    if (l != clen) continue;
    uint32_t j = 0;
    while (j < l && (uint8_t)S.names[a + j] == chrom[j]) ++j;
    if (j == l) ord = k;
  }
  if (ord == S.n_names) return -1;
  const uint64_t key = (uint64_t)ord << 32 | (uint32_t)pos;
  uint32_t lo = 0, hi = S.n_keys;               // the first key >= key
  while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (S.keys[m] < key) lo = m + 1; else hi = m; }
  return lo < S.n_keys && S.keys[lo] == key ? (int32_t)lo : -1;
}
FQ_HD bool fqv_is_snp(const uint8_t *ref, uint32_t ref_len, const uint8_t *alt, uint32_t alt_len) {
  if (ref_len != 1) return false;
  uint32_t a = 0;
  for (uint32_t i = 0; i <= alt_len; ++i)
    if (i == alt_len || alt[i] == ',') {
      if (i - a == 1 && fqv_is_acgt(alt[a]) && fqv_upper(alt[a]) != fqv_upper(ref[0])) return true;
      a = i + 1;
    }
  return false;
}

// ---- a thread per line --------------------------------------------------------------------------------------------------------------------
FQ_HD void fq_vcf_site_line(const FqVcfSiteArgs &A, uint32_t i) {
  const uint8_t *T = A.text;
  const uint32_t beg = i ? A.nl[i - 1] + 1 : A.lo;
  uint32_t end = A.nl[i];
  if (end > A.n) end = A.n;                                  // (never beyond the text, whatever the index says)
  if (end > beg && T[end - 1] == '\r') --end;
  FqVcfLine L;
  L.beg = beg; L.len = end > beg ? end - beg : 0; L.pos = 0; L.flags = 0; L.col9 = end; L.site = -1; L.n_keys = 0; L.key_idx = 0; L.key = 0; L.chrom_len = 0;
  for (uint32_t k = 0; k < FQV_CHROM_INLINE; ++k) L.chrom[k] = 0;
  L.ref = L.alt = 0; L.pad[0] = L.pad[1] = 0;
  uint32_t keep = 0;
  if (end <= beg) L.flags |= FQV_F_EMPTY | (A.use_sites ? 0u : (uint32_t)FQV_F_SITE);
  else {
    if (T[beg] == '#') L.flags |= FQV_F_HASH;
    // the first ten columns: cb[c] where column c begins, ce[c] where it ends
    uint32_t cb[10], ce[10], nc = 0, p = beg;
    cb[0] = beg;
    while (p < end && nc < 9) { if (T[p] == '\t') { ce[nc] = p; ++nc; cb[nc] = p + 1; } ++p; }
    uint32_t n_cols;
    if (nc < 9) { ce[nc] = end; n_cols = nc + 1; }          // the line ended first
    else { n_cols = 10; L.col9 = cb[9]; }                   // (column 9 and whatever follows: k_vcf_geno's)
    if (n_cols < 5) L.flags |= FQV_F_LT5;
    if (n_cols < 10) L.flags |= FQV_F_LT10;
    // CHROM
    const uint32_t clen = ce[0] - cb[0];
    if (clen > FQV_CHROM_INLINE) L.flags |= FQV_F_LONGCHROM;
    else { L.chrom_len = (uint8_t)clen; for (uint32_t k = 0; k < clen; ++k) L.chrom[k] = (char)T[cb[0] + k]; }
    {   // acceptChr: 1 .. 22, chr1 .. chr22
      uint32_t a = cb[0], l = clen;
      if (l >= 3 && T[a] == 'c' && T[a + 1] == 'h' && T[a + 2] == 'r') { a += 3; l -= 3; }
      bool ok = (l == 1 || l == 2) && T[a] >= '1' && T[a] <= '9' && (l == 1 || (T[a + 1] >= '0' && T[a + 1] <= '9'));
      for (uint32_t k = 0; k < clen; ++k) if (T[cb[0] + k] == 0) ok = false;      // (a NUL ends the C string the reader tests: the host decides)
      if (ok) { const int v = l == 1 ? T[a] - '0' : (T[a] - '0') * 10 + (T[a + 1] - '0'); ok = v >= 1 && v <= 22; }
      if (ok) L.flags |= FQV_F_CHROM_OK;
      else for (uint32_t k = 0; k < clen; ++k) if (T[cb[0] + k] == 0) L.flags |= FQV_F_HOST;
    }
    if (n_cols >= 2) {   // POS with atoi's meaning: white space, a sign, digits
      uint32_t q = cb[1];
      const uint32_t qe = ce[1];
      while (q < qe && fqv_is_space(T[q])) ++q;
      bool neg = false;
      if (q < qe && (T[q] == '-' || T[q] == '+')) { neg = T[q] == '-'; ++q; }
      uint64_t v = 0;
      uint32_t nd = 0;
      while (q < qe && T[q] >= '0' && T[q] <= '9') { if (nd < 19) v = v * 10 + (uint64_t)(T[q] - '0'); ++nd; ++q; }
      if (nd > 18) L.flags |= FQV_F_HOST;                    // (beyond what a long holds: the C library's verdict)
      L.pos = (int32_t)(uint32_t)(neg ? (uint64_t)0 - v : v);
    }
    if (n_cols >= 5) {
      const uint32_t rl = ce[3] - cb[3];
      uint32_t al = 0;
      while (cb[4] + al < ce[4] && T[cb[4] + al] != ',') ++al;
      if (rl > 1 || al > 1) L.flags |= FQV_F_INDEL;
      else if (rl == 0 || al == 0) L.flags |= FQV_F_NOALLELE;
      if (rl) L.ref = (char)T[cb[3]];
      if (al) L.alt = (char)T[cb[4]];
      if (A.use_sites) {
        if (!(L.flags & FQV_F_HOST)) {
          const int32_t s = fqv_site_of(A.sites, T + cb[0], clen, L.pos);
          if (s >= 0 && fqv_is_snp(T + cb[3], rl, T + cb[4], ce[4] - cb[4])) { L.site = s; L.flags |= FQV_F_SITE; A.sites.found[s] = 1; }
        }
      } else L.flags |= FQV_F_SITE;
    } else if (!A.use_sites) L.flags |= FQV_F_SITE;
    if (n_cols >= 10) {   // FORMAT: the fields PL, GL, GT -- the first of each -- and the field count
      int32_t at_pl = -1, at_gl = -1, at_gt = -1;
      uint32_t f = 0, a = cb[8];
      for (uint32_t q = cb[8]; q <= ce[8]; ++q)
        if (q == ce[8] || T[q] == ':') {
          if (q - a == 2) {
            const uint8_t x = T[a], y = T[a + 1];
            if (x == 'P' && y == 'L' && at_pl < 0) at_pl = (int32_t)f;
            if (x == 'G' && y == 'L' && at_gl < 0) at_gl = (int32_t)f;
            if (x == 'G' && y == 'T' && at_gt < 0) at_gt = (int32_t)f;
          }
          ++f; a = q + 1;
        }
      L.n_keys = (uint16_t)(f > 0xffffu ? 0xffffu : f);
      int32_t idx = at_pl;
      L.key = FQV_KEY_PL;
      if (idx < 0) { idx = at_gl; L.key = FQV_KEY_GL; }
      if (idx < 0) { idx = at_gt; L.key = FQV_KEY_GT; }
      if (idx < 0) L.flags |= FQV_F_NOKEY;
      else if (idx > 255 || f > 0xffffu || L.key == FQV_KEY_GL) L.flags |= FQV_F_HOST;      // (GL: atof is the host's)
      else L.key_idx = (uint8_t)idx;
    }
    const uint32_t stop = FQV_F_EMPTY | FQV_F_LT5 | FQV_F_LT10 | FQV_F_INDEL | FQV_F_NOALLELE | FQV_F_NOKEY | FQV_F_HOST | FQV_F_LONGCHROM;
    if ((L.flags & FQV_F_SITE) && (L.flags & FQV_F_CHROM_OK) && !(L.flags & stop)) { L.flags |= FQV_F_GENO; keep = 1; }
  }
  A.line[i] = L;
  A.keep[i] = keep;
}
// kept[rank of line i] = i
FQ_HD void fq_vcf_compact_line(const uint32_t *keep, const uint64_t *off, uint32_t *kept, uint32_t i) { if (keep[i]) kept[off[i]] = i; }

// ---- one cell -----------------------------------------------------------------------------------------------------------------------------
// The genotype (-1 .. 2) of the cell that begins at p and ends in front of the next tab or at `end`, or FQV_NEEDS_HOST for a cell that is not plain.
// *cell_end: where the cell ended (the tab's position, or end) when it is plain.  The reader's rules: the phreds capped at 255, the first strict
// minimum below 255, else -1.
FQ_HD int fq_vcf_cell(const uint8_t *T, uint32_t p, uint32_t end, uint32_t n_keys, uint32_t idx, uint32_t key) {
  uint32_t e = p;
  const uint32_t lim = end - p > FQV_CELL_MAX ? p + FQV_CELL_MAX : end;
  uint32_t colons = 0, fs = p, fe = p;      // the selected field [fs, fe)
  bool have = false;
  for (; e < lim && T[e] != '\t'; ++e)
    if (T[e] == ':') {
      if (colons == idx) { fe = e; have = true; }
      ++colons;
      if (colons == idx) fs = e + 1;
    }
  if (e == lim && lim != end) return FQV_NEEDS_HOST;          // longer than a plain cell
  if (e == p) return FQV_NEEDS_HOST;                           // an empty cell
  if (!have) { if (colons == idx) { fe = e; have = true; } }
  const uint32_t len = e - p;
  const bool missing = (len == 1 && T[p] == '.') || (len == 3 && T[p] == '.' && T[p + 1] == '/' && T[p + 2] == '.');
  if (missing) return key == FQV_KEY_GT && idx == 0 ? 0 : FQV_NEEDS_HOST;      // (libVcf: the first value "./.", the others empty -- which ends in a refusal)
  if (colons + 1 != n_keys || !have) return FQV_NEEDS_HOST;
  if (key == FQV_KEY_GT) {
    if (fe - fs != 3) return FQV_NEEDS_HOST;
    const uint8_t a = T[fs], s = T[fs + 1], b = T[fs + 2];
    if (!((a >= '0' && a <= '9') || a == '.') || !((b >= '0' && b <= '9') || b == '.') || (s != '/' && s != '|')) return FQV_NEEDS_HOST;
    const int geno = (a == '.' ? 0 : a - '0') + (b == '.' ? 0 : b - '0');
    return geno == 0 ? 0 : geno == 1 ? 1 : 2;
  }
  if (key != FQV_KEY_PL) return FQV_NEEDS_HOST;
  // digits{1,9} (',' digits{1,9}){2,}
  uint32_t ph[3] = {0, 0, 0}, nv = 0, nd = 0, v = 0;
  for (uint32_t q = fs; q <= fe; ++q) {
    if (q == fe || T[q] == ',') {
      if (nd == 0) return FQV_NEEDS_HOST;
      if (nv < 3) ph[nv] = v;
      ++nv; nd = 0; v = 0;
    } else if (T[q] >= '0' && T[q] <= '9') {
      if (++nd > 9) return FQV_NEEDS_HOST;
      v = v * 10 + (uint32_t)(T[q] - '0');
    } else return FQV_NEEDS_HOST;
  }
  if (nv < 3) return FQV_NEEDS_HOST;
  int g = -1;
  uint32_t best = 255;
  for (int k = 0; k < 3; ++k) { const uint32_t x = ph[k] > 255 ? 255 : ph[k]; if (x < best) { best = x; g = k; } }
  return g;
}
// the cell of sample s of kept row k that begins at p: parsed and stored, or the row's needs_host set
FQ_HD void fq_vcf_cell_store(const FqVcfGenoArgs &A, uint32_t k, const FqVcfLine &L, uint32_t s, uint32_t p, uint32_t end) {
  if (s >= (uint32_t)A.n_sample) { A.needs_host[k] = 1; return; }
  const int g = fq_vcf_cell(A.text, p, end, L.n_keys, L.key_idx, L.key);
  if (g == FQV_NEEDS_HOST) A.needs_host[k] = 1;
  else A.g[(size_t)k * (size_t)A.n_sample + s] = (int8_t)g;
}
// the host loop's walk of kept row k: tab by tab
FQ_HD void fq_vcf_geno_line(const FqVcfGenoArgs &A, uint32_t k) {
  const FqVcfLine L = A.line[A.kept[k]];
  uint32_t end = L.beg + L.len;
  if (end > A.n) end = A.n;
  uint32_t s = 0, p = L.col9;
  if (p >= end) { A.needs_host[k] = 1; return; }
  fq_vcf_cell_store(A, k, L, 0, p, end);
  for (; p < end; ++p)
    if (A.text[p] == '\t') { ++s; if (p + 1 < end) fq_vcf_cell_store(A, k, L, s, p + 1, end); else A.needs_host[k] = 1; }
  if (s + 1 != (uint32_t)A.n_sample) A.needs_host[k] = 1;
}

#if defined(__HIPCC__) && defined(FQ_VCF_KERNELS)
// ---- kernels (launched from fq_device.hip) ----
__global__ void __launch_bounds__(256) k_vcf_site(FqVcfSiteArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < a.n_lines) fq_vcf_site_line(a, i);
}
__global__ void __launch_bounds__(256) k_vcf_compact(const uint32_t *keep, const uint64_t *off, uint32_t *kept, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) fq_vcf_compact_line(keep, off, kept, i);
}
// A workgroup per kept line.  The line's cells lie in text[col9, end); the block walks the 16-byte-aligned tiles that cover them.  Thread t of a tile looks
// at bytes [at, at + 16), at = tile + 16 t: one aligned 16-byte load where that lies inside the text (the text's base is 16-byte aligned), single bytes at
// the text's very end.  Bit j of its mask: byte at + j is a tab inside [col9, end).  The number of tabs in front of a byte is the sample index of the cell
// the byte lies in: the running count of the tiles before, plus the prefix sum over the block's counts (shuffles inside a wavefront, LDS across the four),
// plus the mask's lower bits.  A cell begins behind a tab (and at col9): the thread that holds that tab parses the cell -- fq_vcf_cell reads on from
// global memory, to the cell's end and never beyond `end`.
__global__ void __launch_bounds__(256) k_vcf_geno(FqVcfGenoArgs a) {
  const uint32_t k = blockIdx.x;
  if (k >= a.n_kept) return;
  const FqVcfLine L = a.line[a.kept[k]];
  uint32_t end = L.beg + L.len;
  if (end > a.n) end = a.n;
  const uint32_t col9 = L.col9;
  if (col9 >= end) { if (threadIdx.x == 0) a.needs_host[k] = 1; return; }
  __shared__ uint32_t s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t base = 0;                                           // tabs in front of this tile
  if (threadIdx.x == 0) fq_vcf_cell_store(a, k, L, 0, col9, end);
  for (uint32_t tile = col9 & ~15u; tile < end; tile += FQV_TILE) {      // (uniform over the block)
    const uint32_t at = tile + 16u * threadIdx.x;
    uint32_t m = 0;
    if (at < end) {
      if (at + 16u <= a.n) {
        const FqU4 v = *(const FqU4 *)(a.text + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j) m |= (uint32_t)(((w[q] >> (8 * j)) & 0xffu) == 0x09u) << (4 * q + j);
      } else
        for (uint32_t j = 0; at + j < a.n; ++j) m |= (uint32_t)(a.text[at + j] == '\t') << j;
      if (at + 16u > end) m &= (1u << (end - at)) - 1u;
      if (at < col9) m &= ~((1u << (col9 - at)) - 1u);
    }
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t x = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64); if (lane >= d) x += y; }
    __syncthreads();                                           // (the words of the tile before have been read)
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t before = base + (x - c);
    for (int w = 0; w < wave; ++w) before += s_w[w];
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    while (m) {
      const int j = __ffs((int)m) - 1;
      m &= m - 1;
      ++before;                                                // the cell behind this tab: sample `before`
      if (at + (uint32_t)j + 1u < end) fq_vcf_cell_store(a, k, L, before, at + (uint32_t)j + 1u, end);
      else a.needs_host[k] = 1;                                // (a tab at the line's end: an empty last cell)
    }
  }
  if (threadIdx.x == 0 && base + 1u != (uint32_t)a.n_sample) a.needs_host[k] = 1;
}
#endif

namespace fqdev {
// launchers (fq_device.hip), on the bound state's stream; nothing is waited for
int launch_vcf_site(const FqVcfSiteArgs &a);                   // a thread per line
int launch_vcf_compact(const uint32_t *keep, const uint64_t *off, uint32_t *kept, uint32_t n);
int launch_vcf_geno(const FqVcfGenoArgs &a);                   // a workgroup per kept line
}  // namespace fqdev
