// fq_bamin.h -- BAM records in HBM -> the FASTQ text the front end's tokeniser takes (fq_frontend.h): the third part of `align --bam_in`, behind
// the BGZF member decoder and in front of the line index.  The reference interface this stands in for is the dormant bwa_read_bam
// (libbwa/bwaseqio.c:90-142, switched off at src/BwtMapper.cpp:185-187): name, bases from the 4-bit codes, quality + 33 capped at 126, reverse
// strand records turned back (bwaseqio.c:103-129); where it says nothing -- which records are kept, how mates are found -- the common default of
// `samtools fastq` on collated input.  The per-item bodies below are stated once: fq_device.hip wraps them in kernels, and a build without hipcc
// (tests/emu) gets the launchers as host loops over the same bodies, defined inline here.
//
//   (a) record starts   Record boundaries are a chain of block_size fields, serial by format.  The chain is cut at the BGZF members (<= 64 KiB of
//                       payload each): a wavefront per member looks for the member's first record -- 64 candidate offsets a step against
//                       fq_bam_plausible, first hit by ballot -- and walks on from there, counting.  The guess is then VERIFIED on the host over
//                       16 bytes per member: member k's walk is the chain's only if it began where the chain enters k; where it did not, k is walked
//                       again from the true offset (a repair), and members the chain jumps over hold no start whatever they guessed.  The result
//                       is exactly the chain from the first record behind the header: a wrong guess costs a relaunch, never a record.  Past
//                       FQB_MAX_REPAIRS relaunches one thread walks the rest.  One scan over the counts, and a second pass writes the starts.
//   (b) keep, pair      a thread per record: kept unless secondary / supplementary; a scan ranks the kept; a thread per pair (per record of a
//                       single-end stream) checks flags and names, says which record goes to which side and how long its text is
//   (c) fill            a wavefront per (pair, side): the four lines, a dword of destination a lane and step
//   (b') collate        (`--collate`; in place of (b)'s pairing) mates are matched by name across the whole stream: the records that wait for their mate
//                       are held in HBM from chunk to chunk.  Per chunk: a hash of every kept record's name; held and kept records together sorted
//                       stably by hash (fq_sort.h); a thread per run of equal hashes walks it in ordinal order and applies the serial definition
//                        among byte-equal names; a scan over the completing records gives the pairs their places; after the fill the
//                       records still waiting are gathered, a wavefront each, into the other half of the held store
//   (b'') tags          (`--bam_rg`, `--bam_oq`; in place of (b)'s keep) a thread per record walks the auxiliary fields (SAM specification 4.2.4): kept is
//                       then "neither secondary nor supplementary, and its RG:Z is one of the wanted IDs"; where OQ:Z is to be read, its offset in the
//                       record goes with the record -- to its unit, and into the held store -- and the fill takes the quality line from there
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "fq_kernels.h"

#define FQB_NONE 0xffffffffu
#define FQB_MAX_BLOCK (1u << 28)          // a block_size (or l_seq) above this is not a record's
#define FQB_MAX_REPAIRS 64                // relaunches of a member's walk in one chunk; then the serial walk
enum { FQB_SEG_OK = 0, FQB_SEG_CUT = 1, FQB_SEG_CORRUPT = 2 };      // how a member's walk ended: at the member's end; at a record the payload's end cuts off; at a block_size that is none
// what a record is refused for; a refusal is the pair (record ordinal, kind) as ordinal << FQB_KIND_BITS | kind, and the stream's is the smallest
enum { FQB_BAD_MIXED = 1, FQB_BAD_LSEQ0 = 2, FQB_BAD_FIELDS = 3, FQB_BAD_NAME = 4, FQB_BAD_MATES = 5, FQB_BAD_NAMES = 6, FQB_BAD_DUP = 7, FQB_BAD_AUX = 8, FQB_BAD_OQ = 9 };
#define FQB_KIND_BITS 4
#define FQB_NO_BAD 0xffffffffffffffffull

// seg[0 .. n_seg]: where the members begin in the payload (seg[0]: the first record; seg[n_seg] = n); per member: first (where its walk began, or
// FQB_NONE), last_next (the offset behind its last record), count, flag
struct FqBamChainArgs {
  const uint8_t *pay; uint32_t n; const uint32_t *seg; uint32_t n_seg; int32_t n_ref;
  uint32_t *first, *last_next, *count, *flag;
  const uint64_t *base; uint32_t *starts;       // (second pass) base[k]: the records in front of member k
};
struct FqBamPairArgs {
  const uint8_t *pay; const uint32_t *starts; uint32_t n_rec;
  uint32_t *kept; const uint64_t *kord; uint32_t *kidx;        // kept[i] 0/1, its scan, the kept records' indices
  uint32_t n_units; int32_t paired; uint64_t ord0;             // units: pairs, or single records; ord0: the stream's records in front of this chunk's
  uint32_t *src[2], *len[2];                                   // per unit and side: the record's offset, its text's length
  uint64_t *bad;
  const uint32_t *roq; uint32_t *oq[2];                        // (--bam_oq; or null) per record: the offset of its OQ value in the record, 0: none; per unit and side: the same
};
// (b'') sel (or null: every record is selected): the wanted IDs as dwords -- their count, their lengths, then their bytes one behind the other
struct FqBamTagArgs {
  const uint8_t *pay; const uint32_t *starts; uint32_t n_rec; uint64_t ord0;
  const uint32_t *sel; int32_t use_oq;
  uint32_t *kept, *roq, *unsel, *hasoq;                        // per record: kept 0/1; the OQ value's offset (0: none, or not asked for); not selected 0/1; kept with an OQ value 0/1
  uint64_t *bad;
};
// from[e] (collation; or null): per unit, 1 where side e's record lies in the held store -- src[e][u] is then its index there, held + hoff[index] the record
struct FqBamFillArgs { const uint8_t *pay; const uint32_t *src[2]; const uint64_t *off[2]; uint8_t *text[2]; uint32_t n_units; int32_t n_sides; uint64_t total[2];      // total[e] = off[e][n_units]
                       const uint8_t *held; const uint64_t *hoff; const uint8_t *from[2];
                       const uint32_t *oq[2]; };      // oq[e] (--bam_oq; or null): per unit, the offset of the OQ value in side e's record, 0: none
// Collation.  Candidates of a chunk: the held records [0, n_held) -- older, in ordinal order -- then the chunk's kept records in chunk order.
enum { FQC_WAIT = 0, FQC_PAIR = 1, FQC_USED = 2, FQC_BAD = 3 };      // a candidate: waits for its mate; completes a pair with mate[c]; is the earlier record of a pair; is refused
struct FqBamCollateArgs {
  const uint8_t *pay; const uint32_t *starts, *kidx; uint32_t n_kept; uint64_t ord0;      // the chunk's kept records
  const uint8_t *held; const uint64_t *hoff, *hkey, *hord; uint32_t n_held;                // the held store: records, their offsets, hashes, ordinals
  uint32_t n; uint64_t mask;                                                               // n = n_held + n_kept; the hash's bits that group
  uint64_t *hash, *key;                                                                    // per candidate: the name's hash; hash & mask, the sort's input
  uint32_t *st, *mate;                                                                     // per candidate: FQC_*; the candidate an FQC_PAIR completes
  const uint64_t *skey; const uint32_t *perm;                                              // the sort's output
  uint32_t *flag; const uint64_t *uidx;                                                    // per kept record: completes a pair; the scan: its unit
  uint8_t *from[2]; uint32_t *src[2], *len[2];                                             // per unit and side, as FqBamFillArgs / FqBamPairArgs
  uint64_t *bad;
  uint32_t *surv, *rlen; const uint64_t *sidx, *soff;                                      // per candidate: still waiting; its bytes; their scans
  uint8_t *nheld; uint64_t *noff, *nkey, *nord;                                            // the other half of the held store
  const uint32_t *roq, *hoq; uint32_t *oq[2], *noq;                                        // (--bam_oq; or all null) the OQ offsets: per record of the chunk, per held record; per unit and side; of the other half
};

FQ_HD uint32_t fqb_ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
FQ_HD uint32_t fqb_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// what block_size must cover: the fixed fields, the name, the CIGAR, the packed bases and the qualities
FQ_HD uint64_t fqb_min_block(uint32_t l_name, uint32_t n_cig, uint32_t l_seq) { return 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq; }

// ---- (a) ----
// Could a record begin at c?  Its fixed fields against its block_size; false too when fewer than 36 bytes are left.  *next: where it ends.
FQ_HD bool fq_bam_plausible1(const uint8_t *pay, uint32_t n, uint64_t c, int32_t n_ref, uint64_t *next) {
  if (c + 36 > n) return false;
  const uint8_t *r = pay + c;
  const uint32_t bs = fqb_ld32(r), l_name = r[12], n_cig = fqb_ld16(r + 16), l_seq = fqb_ld32(r + 20);
  const int32_t ref = (int32_t)fqb_ld32(r + 4), nref = (int32_t)fqb_ld32(r + 24);
  if (bs > FQB_MAX_BLOCK || l_seq > FQB_MAX_BLOCK || bs < fqb_min_block(l_name, n_cig, l_seq)) return false;
  if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref) return false;
  if (l_name < 2) return false;
  const uint64_t nul = c + 36 + l_name - 1;
  if (nul < n && pay[nul] != 0) return false;
  *next = c + 4 + bs;
  return true;
}
// ... and the two records behind it, as far as the payload shows their fixed fields
FQ_HD bool fq_bam_plausible(const uint8_t *pay, uint32_t n, uint32_t c, int32_t n_ref) {
  uint64_t p = c, nx = 0;
  if (!fq_bam_plausible1(pay, n, p, n_ref, &nx)) return false;
  for (int d = 0; d < 2; ++d) {
    p = nx;
    if (p + 36 > n) return true;
    if (!fq_bam_plausible1(pay, n, p, n_ref, &nx)) return false;
  }
  return true;
}
// The records that begin in member k, from p on (seg[k] <= p): counted, and written to out when it is given.  Every step moves on by 36 bytes at
// least and stays inside the payload, whatever the bytes say.
FQ_HD void fq_bam_walk_seg(const FqBamChainArgs &a, uint32_t k, uint32_t p, uint32_t *out) {
  const uint32_t end = a.seg[k + 1], p0 = p;
  uint32_t cnt = 0, flag = FQB_SEG_OK;
  while (p < end) {
    if ((uint64_t)p + 4 > a.n) { flag = FQB_SEG_CUT; break; }
    const uint32_t bs = fqb_ld32(a.pay + p);
    if (bs < 32 || bs > FQB_MAX_BLOCK) { flag = FQB_SEG_CORRUPT; break; }
    if ((uint64_t)p + 4 + bs > a.n) { flag = FQB_SEG_CUT; break; }
    if (out) out[cnt] = p;
    ++cnt; p += 4 + bs;
  }
  if (!out) { a.first[k] = p0; a.last_next[k] = p; a.count[k] = cnt; a.flag[k] = flag; }
}
FQ_HD void fq_bam_seg_none(const FqBamChainArgs &a, uint32_t k) { a.first[k] = FQB_NONE; a.last_next[k] = FQB_NONE; a.count[k] = 0; a.flag[k] = FQB_SEG_OK; }
// second pass, a thread per member: the starts of its records at their places
FQ_HD void fq_bam_starts_thread(const FqBamChainArgs &a, uint32_t k) {
  if (a.count[k]) fq_bam_walk_seg(a, k, a.first[k], a.starts + a.base[k]);
}
// the chain from p (in member k) to the payload's end on one thread: what the members' guesses are held to, and what is left when too many were wrong
FQ_HD void fq_bam_chain_serial(const FqBamChainArgs &a, uint32_t k, uint32_t p) {
  while (k < a.n_seg) {
    fq_bam_walk_seg(a, k, p, nullptr);
    p = a.last_next[k];
    const bool ended = a.flag[k] != FQB_SEG_OK || p >= a.n;
    ++k;
    while (k < a.n_seg && (ended || a.seg[k + 1] <= p)) { fq_bam_seg_none(a, k); ++k; }
  }
}

// ---- (b) ----
FQ_HD void fq_bam_keep_thread(const FqBamPairArgs &a, uint32_t i) { a.kept[i] = (fqb_ld16(a.pay + a.starts[i] + 18) & 0x900u) ? 0u : 1u; }
FQ_HD void fq_bam_kidx_thread(const FqBamPairArgs &a, uint32_t i) { if (a.kept[i]) a.kidx[a.kord[i]] = i; }
FQ_HD uint64_t fqb_bad(uint64_t ord, uint32_t kind) { return ord << FQB_KIND_BITS | kind; }
FQ_HD uint64_t fqb_bad_ord(uint64_t bad) { return bad >> FQB_KIND_BITS; }
FQ_HD uint32_t fqb_bad_kind(uint64_t bad) { return (uint32_t)(bad & ((1u << FQB_KIND_BITS) - 1u)); }
FQ_HD uint64_t fqb_min64(uint64_t x, uint64_t y) { return x < y ? x : y; }
// what one kept record is refused for on its own (FQB_NO_BAD: nothing)
FQ_HD uint64_t fq_bam_record_check(const uint8_t *r, uint64_t ord, int32_t paired) {
  const uint32_t bs = fqb_ld32(r), l_name = r[12], n_cig = fqb_ld16(r + 16), flag = fqb_ld16(r + 18), l_seq = fqb_ld32(r + 20);
  if (((flag & 1u) != 0) != (paired != 0)) return fqb_bad(ord, FQB_BAD_MIXED);
  if (l_seq == 0) return fqb_bad(ord, FQB_BAD_LSEQ0);
  if (l_seq > FQB_MAX_BLOCK || bs < fqb_min_block(l_name, n_cig, l_seq)) return fqb_bad(ord, FQB_BAD_FIELDS);      // (the fill reads name, bases and qualities inside the record only)
  if (l_name < 2) return fqb_bad(ord, FQB_BAD_NAME);
  for (uint32_t j = 0; j + 1 < l_name; ++j) if (r[36 + j] < 0x21 || r[36 + j] > 0x7e) return fqb_bad(ord, FQB_BAD_NAME);
  return FQB_NO_BAD;
}
FQ_HD uint32_t fq_bam_text_len(const uint8_t *r) { return (uint32_t)r[12] - 1u + 2u * fqb_ld32(r + 20) + 6u; }
// a pair (kept records 2u, 2u + 1) or a single-end record: its refusal, or FQB_NO_BAD
FQ_HD uint64_t fq_bam_unit_thread(const FqBamPairArgs &a, uint32_t u) {
  if (!a.paired) {
    const uint32_t i = a.kidx[u], s = a.starts[i];
    const uint64_t bad = fq_bam_record_check(a.pay + s, a.ord0 + i, 0);
    a.src[0][u] = s; a.len[0][u] = bad == FQB_NO_BAD ? fq_bam_text_len(a.pay + s) : 0;
    if (a.roq) a.oq[0][u] = a.roq[i];
    return bad;
  }
  const uint32_t ia = a.kidx[2 * u], ib = a.kidx[2 * u + 1], sa = a.starts[ia], sb = a.starts[ib];
  const uint8_t *ra = a.pay + sa, *rb = a.pay + sb;
  uint64_t bad = fqb_min64(fq_bam_record_check(ra, a.ord0 + ia, 1), fq_bam_record_check(rb, a.ord0 + ib, 1));
  const uint32_t fa = fqb_ld16(ra + 18) & 0xc0u, fb = fqb_ld16(rb + 18) & 0xc0u;
  const bool a_first = fa == 0x40u && fb == 0x80u;
  if (bad == FQB_NO_BAD && !a_first && !(fa == 0x80u && fb == 0x40u)) bad = fqb_bad(a.ord0 + ia, FQB_BAD_MATES);      // (two records that stand on their own: are they a pair?)
  if (bad == FQB_NO_BAD) {
    bool same = ra[12] == rb[12];
    for (uint32_t j = 0; same && j < ra[12]; ++j) same = ra[36 + j] == rb[36 + j];
    if (!same) bad = fqb_bad(a.ord0 + ia, FQB_BAD_NAMES);
  }
  a.src[0][u] = a_first ? sa : sb; a.src[1][u] = a_first ? sb : sa;
  if (a.roq) { a.oq[0][u] = a.roq[a_first ? ia : ib]; a.oq[1][u] = a.roq[a_first ? ib : ia]; }
  a.len[0][u] = bad == FQB_NO_BAD ? fq_bam_text_len(a_first ? ra : rb) : 0;
  a.len[1][u] = bad == FQB_NO_BAD ? fq_bam_text_len(a_first ? rb : ra) : 0;
  return bad;
}

// ---- (b'') ----
// The auxiliary fields of record r, which lies whole in the payload: from behind the qualities to 4 + block_size, a field after the other -- two tag
// bytes, a type, a value (A c C: 1 byte; s S: 2; i I f: 4; Z H: up to and including the first NUL inside the area; B: a subtype of cCsSiIf, a 32-bit
// count, count x size bytes, in 64 bits).  The first RG and the first OQ are noted: the value's offset in the record and its length without the
// NUL.  False (FQB_BAD_AUX) unless the walk ends exactly at the area's end: an unknown type or subtype, a value that runs beyond the area, a Z / H
// without NUL, one or two stray bytes, a first RG or OQ whose type is not Z.  Every step moves on by three bytes at least and reads inside the area only.
struct FqBamAux { uint32_t rg, rg_len, oq, oq_len; };      // (offset 0: the record has none)
FQ_HD uint32_t fqb_aux_size(uint8_t t) { return t == 'A' || t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : t == 'i' || t == 'I' || t == 'f' ? 4u : 0u; }
FQ_HD bool fq_bam_aux_walk(const uint8_t *r, FqBamAux *x) {
  x->rg = x->rg_len = x->oq = x->oq_len = 0;
  const uint64_t end = 4ull + fqb_ld32(r);
  uint64_t p = 4ull + fqb_min_block(r[12], fqb_ld16(r + 16), fqb_ld32(r + 20));
  if (p > end) return false;
  while (p < end) {
    if (p + 3 > end) return false;
    const uint8_t t0 = r[p], t1 = r[p + 1], ty = r[p + 2];
    const bool is_rg = t0 == 'R' && t1 == 'G' && !x->rg, is_oq = t0 == 'O' && t1 == 'Q' && !x->oq;
    if ((is_rg || is_oq) && ty != 'Z') return false;
    p += 3;
    if (ty == 'Z' || ty == 'H') {
      uint64_t q = p;
      while (q < end && r[q]) ++q;
      if (q >= end) return false;
      if (is_rg) { x->rg = (uint32_t)p; x->rg_len = (uint32_t)(q - p); }
      if (is_oq) { x->oq = (uint32_t)p; x->oq_len = (uint32_t)(q - p); }
      p = q + 1;
    } else if (ty == 'B') {
      if (p + 5 > end) return false;
      const uint64_t sz = fqb_aux_size(r[p]);
      if (!sz || r[p] == 'A') return false;
      p += 5 + sz * (uint64_t)fqb_ld32(r + p + 1);
    } else {
      const uint32_t sz = fqb_aux_size(ty);
      if (!sz) return false;
      p += sz;
    }
    if (p > end) return false;
  }
  return true;
}
// is the value one of the wanted IDs, in length and in bytes?
FQ_HD bool fq_bam_rg_wanted(const uint32_t *sel, const uint8_t *v, uint32_t len) {
  const uint32_t n = sel[0];
  const uint8_t *b = (const uint8_t *)(sel + 1 + n);
  for (uint32_t k = 0; k < n; b += sel[1 + k], ++k) {
    if (sel[1 + k] != len) continue;
    uint32_t j = 0;
    while (j < len && b[j] == v[j]) ++j;
    if (j == len) return true;
  }
  return false;
}
// a record that is neither secondary nor supplementary, walked: selected or not, where its OQ value lies, whether that fits the read.  *kept, *oq (0: none,
// or not asked for), *unsel as FqBamTagArgs has them per record.  Where the walk fails, the RG it met in front of what stopped it says selected or not: a
// selected record stays kept, and its own check may refuse it for less.
FQ_HD uint32_t fq_bam_tags_record(const uint8_t *r, const uint32_t *sel, int use_oq, uint32_t *kept, uint32_t *oq, uint32_t *unsel) {
  *oq = 0;
  FqBamAux x;
  const bool good = fq_bam_aux_walk(r, &x);
  const bool selected = !sel || (x.rg && fq_bam_rg_wanted(sel, r + x.rg, x.rg_len));
  *kept = selected ? 1u : 0u; *unsel = selected ? 0u : 1u;
  if (!good) return FQB_BAD_AUX;
  if (!selected) return 0;
  if (use_oq && x.oq) {
    if (x.oq_len != fqb_ld32(r + 20)) return FQB_BAD_OQ;
    for (uint32_t j = 0; j < x.oq_len; ++j) if (r[x.oq + j] < 0x21 || r[x.oq + j] > 0x7e) return FQB_BAD_OQ;
    *oq = x.oq;
  }
  return 0;
}
FQ_HD uint64_t fq_bam_tags_thread(const FqBamTagArgs &a, uint32_t i) {
  const uint8_t *r = a.pay + a.starts[i];
  uint32_t kept = 0, oq = 0, unsel = 0, kind = 0;
  if (!(fqb_ld16(r + 18) & 0x900u)) kind = fq_bam_tags_record(r, a.sel, a.use_oq, &kept, &oq, &unsel);
  a.kept[i] = kept; a.roq[i] = oq; a.unsel[i] = unsel; a.hasoq[i] = oq ? 1u : 0u;
  return kind ? fqb_bad(a.ord0 + i, kind) : FQB_NO_BAD;
}

// ---- (c) ----
// byte j of the record's four lines "@name\nSEQ\n+\nQUAL\n" (nm name bytes, l bases); oq (or null): the record's OQ value, l bytes that are Phred+33 as they stand
FQ_HD uint8_t fq_bam_text_byte(const uint8_t *r, uint32_t nm, uint32_t l, uint32_t n_cig, bool rev, uint32_t j, const uint8_t *oq) {
  if (j == 0) return '@';
  if (j <= nm) return r[36 + j - 1];
  j -= nm + 1;
  if (j == 0) return '\n';
  const uint8_t *seq = r + 36 + nm + 1 + 4 * n_cig;
  if (j <= l) {
    const uint32_t b = rev ? l - j : j - 1;
    const uint32_t code = (seq[b >> 1] >> ((~b & 1u) << 2)) & 15u;
    return (uint8_t)(rev ? "=TGKCYSBAWRDMHVN" : "=ACMGRSVTWYHKDBN")[code];
  }
  j -= l + 1;
  if (j == 0) return '\n';
  if (j == 1) return '+';
  if (j == 2) return '\n';
  j -= 3;
  if (j < l) {
    if (oq) return oq[rev ? l - 1 - j : j];
    const uint32_t q = (seq + (l + 1) / 2)[rev ? l - 1 - j : j];
    return (uint8_t)(q > 93u ? 126u : q + 33u);        // min(q + 33, 126) (bwaseqio.c:118); a missing quality (0xff) is '~' as well
  }
  return '\n';
}
// lane of the wavefront of (unit u, side e).  The text lies at any alignment: a lane takes an aligned dword of the destination a step, whole dwords
// inside the record's text are stored as dwords (256 contiguous bytes a wavefront and step), the at most three bytes at either end as bytes.
FQ_HD const uint8_t *fq_bam_fill_rec(const FqBamFillArgs &a, int e, uint32_t u) { return a.from[e] && a.from[e][u] ? a.held + a.hoff[a.src[e][u]] : a.pay + a.src[e][u]; }
FQ_HD const uint8_t *fq_bam_fill_oq(const FqBamFillArgs &a, int e, uint32_t u, const uint8_t *r) { return a.oq[e] && a.oq[e][u] ? r + a.oq[e][u] : nullptr; }
FQ_HD void fq_bam_fill_lane(const FqBamFillArgs &a, uint32_t u, int e, uint32_t lane) {
  const uint8_t *r = fq_bam_fill_rec(a, e, u), *oq = fq_bam_fill_oq(a, e, u, r);
  const uint32_t nm = (uint32_t)r[12] - 1u, n_cig = fqb_ld16(r + 16), l = fqb_ld32(r + 20);
  const bool rev = (fqb_ld16(r + 18) & 0x10u) != 0;
  const uint64_t len = a.off[e][u + 1] - a.off[e][u];
  uint8_t *d = a.text[e] + a.off[e][u];
  const uint32_t mis = (uint32_t)((uintptr_t)d & 3u);
  for (uint64_t w = lane;; w += 64) {
    const int64_t j0 = (int64_t)(4 * w) - (int64_t)mis;
    if (j0 >= (int64_t)len) break;
    if (j0 >= 0 && (uint64_t)j0 + 4 <= len) {
      uint32_t v = 0;
      for (uint32_t t = 0; t < 4; ++t) v |= (uint32_t)fq_bam_text_byte(r, nm, l, n_cig, rev, (uint32_t)j0 + t, oq) << (8 * t);
      *(uint32_t *)(d + j0) = v;
    } else {
      for (int64_t j = j0 < 0 ? 0 : j0; j < j0 + 4 && j < (int64_t)len; ++j) d[j] = fq_bam_text_byte(r, nm, l, n_cig, rev, (uint32_t)j, oq);
    }
  }
}
// The other form (A/B, FASTQUICK_BAM_FILL=pieces): a thread per sixteen aligned destination bytes of side e, as fq_sort.h's fq_bam_gather_piece16 -- the unit
// that holds the piece's first byte by bisection over off[e], then on through the units; a whole piece inside the text is stored as four dwords.
FQ_HD void fq_bam_fill_piece(const FqBamFillArgs &a, int e, uint64_t t) {
  const uint32_t mis = (uint32_t)((uintptr_t)a.text[e] & 15u);
  const int64_t lo_b = (int64_t)(16 * t) - (int64_t)mis;                    // text offsets [lo_b, lo_b + 16) cut to [0, total)
  uint64_t b = lo_b < 0 ? 0 : (uint64_t)lo_b;
  const uint64_t hi = (uint64_t)(lo_b + 16) < a.total[e] ? (uint64_t)(lo_b + 16) : a.total[e];
  if (lo_b + 16 <= 0 || b >= hi) return;
  uint32_t lo = 0, up = a.n_units;                                          // the last unit with off <= b
  while (up - lo > 1) { const uint32_t m = lo + ((up - lo) >> 1); if (a.off[e][m] <= b) lo = m; else up = m; }
  uint32_t u = lo, w[4] = {0, 0, 0, 0};
  const bool whole = lo_b >= 0 && hi == (uint64_t)lo_b + 16;
  while (b < hi) {
    while (u + 1 < a.n_units && a.off[e][u + 1] <= b) ++u;
    const uint64_t uend = a.off[e][u + 1] < hi ? a.off[e][u + 1] : hi;
    const uint8_t *r = fq_bam_fill_rec(a, e, u), *oq = fq_bam_fill_oq(a, e, u, r);
    const uint32_t nm = (uint32_t)r[12] - 1u, n_cig = fqb_ld16(r + 16), l = fqb_ld32(r + 20);
    const bool rev = (fqb_ld16(r + 18) & 0x10u) != 0;
    for (; b < uend; ++b) {
      const uint8_t c = fq_bam_text_byte(r, nm, l, n_cig, rev, (uint32_t)(b - a.off[e][u]), oq);
      if (whole) { const uint32_t k = (uint32_t)(b - (uint64_t)lo_b); w[k >> 2] |= (uint32_t)c << (8 * (k & 3)); } else a.text[e][b] = c;
    }
  }
  if (whole) { uint32_t *d = (uint32_t *)(a.text[e] + lo_b); d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3]; }
}
FQ_HD uint64_t fq_bam_fill_pieces(const FqBamFillArgs &a, int e) { return a.total[e] ? (a.total[e] + ((uintptr_t)a.text[e] & 15u) + 15) / 16 : 0; }

// ---- (b') collation ----
FQ_HD const uint8_t *fqc_rec(const FqBamCollateArgs &a, uint32_t c) { return c < a.n_held ? a.held + a.hoff[c] : a.pay + a.starts[a.kidx[c - a.n_held]]; }
FQ_HD uint64_t fqc_ord(const FqBamCollateArgs &a, uint32_t c) { return c < a.n_held ? a.hord[c] : a.ord0 + a.kidx[c - a.n_held]; }
FQ_HD uint32_t fqc_oq(const FqBamCollateArgs &a, uint32_t c) { return c < a.n_held ? a.hoq[c] : a.roq[a.kidx[c - a.n_held]]; }      // (where a.roq is given)
// 64 bits of l_read_name and the name's bytes (FNV-1a, then a finaliser so that any k low bits group evenly).  The hash only groups: equality is
// always l_read_name and a byte compare (fqc_same_name).
FQ_HD uint64_t fqc_hash(const uint8_t *r) {
  uint64_t h = 0xcbf29ce484222325ull;
  const uint32_t l_name = r[12];
  h = (h ^ l_name) * 0x100000001b3ull;
  for (uint32_t j = 0; j < l_name; ++j) h = (h ^ r[36 + j]) * 0x100000001b3ull;
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
FQ_HD bool fqc_same_name(const uint8_t *x, const uint8_t *y) {
  if (x[12] != y[12]) return false;
  for (uint32_t j = 0; j < x[12]; ++j) if (x[36 + j] != y[36 + j]) return false;
  return true;
}
// candidate c: its hash and sort key; a kept record of the chunk is checked on its own (rule 3).  Returns its refusal, or FQB_NO_BAD.
FQ_HD uint64_t fq_bam_ckey_thread(const FqBamCollateArgs &a, uint32_t c) {
  a.mate[c] = FQB_NONE;
  if (c < a.n_held) { a.hash[c] = a.hkey[c]; a.key[c] = a.hkey[c] & a.mask; a.st[c] = FQC_WAIT; return FQB_NO_BAD; }
  a.flag[c - a.n_held] = 0;
  const uint8_t *r = fqc_rec(a, c);
  uint64_t bad = fq_bam_record_check(r, fqc_ord(a, c), 1);
  const uint32_t side = fqb_ld16(r + 18) & 0xc0u;
  if (bad == FQB_NO_BAD && side != 0x40u && side != 0x80u) bad = fqb_bad(fqc_ord(a, c), FQB_BAD_MATES);
  const uint64_t h = bad == FQB_NO_BAD ? fqc_hash(r) : 0;      // (a refused record's name may not lie inside it)
  a.hash[c] = h; a.key[c] = h & a.mask; a.st[c] = bad == FQB_NO_BAD ? FQC_WAIT : FQC_BAD;
  return bad;
}
// Sorted place i: where a run of equal keys begins, its thread walks the run -- stable sort: in ordinal order -- and applies rule 4.  The nearest
// earlier record of the same name decides: waiting with the other side bit, the two are a pair; waiting with the same side bit, this one is
// refused; itself the later record of a pair (or no such record), this one waits.  Held records are never a pair among themselves, so only the
// chunk's records look back.  Returns the run's first refusal, or FQB_NO_BAD.
FQ_HD uint64_t fq_bam_cmatch_thread(const FqBamCollateArgs &a, uint32_t i) {
  if (i && a.skey[i - 1] == a.skey[i]) return FQB_NO_BAD;
  uint64_t bad = FQB_NO_BAD;
  for (uint32_t t = i; t < a.n && a.skey[t] == a.skey[i]; ++t) {
    const uint32_t c = a.perm[t];
    if (c < a.n_held || a.st[c] == FQC_BAD) continue;
    const uint64_t h = a.hash[c];
    const uint8_t *r = fqc_rec(a, c);
    for (uint32_t s = t; s > i; --s) {
      const uint32_t w = a.perm[s - 1];
      if (a.hash[w] != h || a.st[w] == FQC_BAD) continue;
      const uint8_t *q = fqc_rec(a, w);
      if (!fqc_same_name(q, r)) continue;
      if (a.st[w] == FQC_WAIT) {
        if (((fqb_ld16(q + 18) ^ fqb_ld16(r + 18)) & 0xc0u) == 0) { a.st[c] = FQC_BAD; bad = fqb_min64(bad, fqb_bad(fqc_ord(a, c), FQB_BAD_DUP)); }
        else { a.st[c] = FQC_PAIR; a.mate[c] = w; a.st[w] = FQC_USED; a.flag[c - a.n_held] = 1; }
      }
      break;
    }
  }
  return bad;
}
// kept record k of the chunk, where it completes a pair: the unit's two sides, the 0x40 record first (as fq_bam_unit_thread for adjacent mates)
FQ_HD void fq_bam_cunit_thread(const FqBamCollateArgs &a, uint32_t k) {
  if (!a.flag[k]) return;
  const uint32_t u = (uint32_t)a.uidx[k], c = a.n_held + k, w = a.mate[c];
  const bool c_first = (fqb_ld16(fqc_rec(a, c) + 18) & 0xc0u) == 0x40u;
  for (int e = 0; e < 2; ++e) {
    const uint32_t x = (e == 0) == c_first ? c : w;
    a.from[e][u] = x < a.n_held ? 1 : 0;
    a.src[e][u] = x < a.n_held ? x : a.starts[a.kidx[x - a.n_held]];
    a.len[e][u] = fq_bam_text_len(fqc_rec(a, x));
    if (a.roq) a.oq[e][u] = fqc_oq(a, x);
  }
}
// what stays: candidate c still waits -- its bytes (block_size included) -- or does not
FQ_HD void fq_bam_cmark_thread(const FqBamCollateArgs &a, uint32_t c) {
  const bool w = a.st[c] == FQC_WAIT;
  a.surv[c] = w ? 1u : 0u; a.rlen[c] = w ? 4u + fqb_ld32(fqc_rec(a, c)) : 0u;
}
// lane of the wavefront of candidate c: a waiting record into the other half of the held store, sixty-four bytes a step (as fq_sort.h's fq_bam_gather_record_lane)
FQ_HD void fq_bam_chold_lane(const FqBamCollateArgs &a, uint32_t c, uint32_t lane) {
  if (!a.surv[c]) return;
  const uint8_t *s = fqc_rec(a, c);
  const uint64_t d0 = a.soff[c], len = a.rlen[c];
  for (uint64_t k = lane; k < len; k += 64) a.nheld[d0 + k] = s[k];
  if (lane == 0) { const uint64_t j = a.sidx[c]; a.noff[j] = d0; a.nkey[j] = a.hash[c]; a.nord[j] = fqc_ord(a, c); if (a.roq) a.noq[j] = fqc_oq(a, c); }
}
FQ_HD uint64_t fqc_mask(int bits) { return bits <= 0 ? 0ull : bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }
#define FQC_HASH_BITS 32      // the bits of the hash that group by default: four passes of the sort; the records of equal hashes meet in one run, and there a byte compare decides

namespace fqdev {
#if defined(__HIPCC__)
int launch_bam_guess(const FqBamChainArgs &a);                                  // a wavefront per member: first / last_next / count / flag
int launch_bam_rewalk(const FqBamChainArgs &a, uint32_t k, uint32_t p, int to_end);   // one thread: member k from p (to_end: the chain from there to the payload's end)
int launch_bam_starts(const FqBamChainArgs &a);                                 // a thread per member
int launch_bam_keep(const FqBamPairArgs &a);                                    // a thread per record
int launch_bam_kidx(const FqBamPairArgs &a);
int launch_bam_tags(const FqBamTagArgs &a);                                     // a thread per record; *a.bad lowered to the first refusal of kinds 8 / 9
int launch_bam_units(const FqBamPairArgs &a);                                   // a thread per pair; *a.bad lowered to the first refusal
int launch_bam_fill(const FqBamFillArgs &a);                                    // a wavefront per (pair, side) (FASTQUICK_BAM_FILL=pieces: a thread per sixteen destination bytes, A/B)
int bam_hash_bits();                                                            // FASTQUICK_BAM_HASH_BITS=k (0..64; tests: many names in one run), or FQC_HASH_BITS
int launch_bam_ckeys(const FqBamCollateArgs &a);                                // a thread per candidate; *a.bad lowered
int launch_bam_cmatch(const FqBamCollateArgs &a);                               // a thread per sorted place (per run); *a.bad lowered
int launch_bam_cunits(const FqBamCollateArgs &a);                               // a thread per kept record
int launch_bam_cmark(const FqBamCollateArgs &a);                                // a thread per candidate
int launch_bam_chold(const FqBamCollateArgs &a);                                // a wavefront per candidate
#else
inline int launch_bam_guess(const FqBamChainArgs &a) {
  for (uint32_t k = 0; k < a.n_seg; ++k) {
    uint32_t c = a.seg[k];
    if (k) { while (c < a.seg[k + 1] && !fq_bam_plausible(a.pay, a.n, c, a.n_ref)) ++c; }
    if (c < a.seg[k + 1]) fq_bam_walk_seg(a, k, c, nullptr); else fq_bam_seg_none(a, k);
  }
  return 0;
}
inline int launch_bam_rewalk(const FqBamChainArgs &a, uint32_t k, uint32_t p, int to_end) { if (to_end) fq_bam_chain_serial(a, k, p); else fq_bam_walk_seg(a, k, p, nullptr); return 0; }
inline int launch_bam_starts(const FqBamChainArgs &a) { for (uint32_t k = 0; k < a.n_seg; ++k) fq_bam_starts_thread(a, k); return 0; }
inline int launch_bam_keep(const FqBamPairArgs &a) { for (uint32_t i = 0; i < a.n_rec; ++i) fq_bam_keep_thread(a, i); return 0; }
inline int launch_bam_kidx(const FqBamPairArgs &a) { for (uint32_t i = 0; i < a.n_rec; ++i) fq_bam_kidx_thread(a, i); return 0; }
inline int launch_bam_tags(const FqBamTagArgs &a) { for (uint32_t i = 0; i < a.n_rec; ++i) *a.bad = fqb_min64(*a.bad, fq_bam_tags_thread(a, i)); return 0; }
inline int launch_bam_units(const FqBamPairArgs &a) { for (uint32_t u = 0; u < a.n_units; ++u) *a.bad = fqb_min64(*a.bad, fq_bam_unit_thread(a, u)); return 0; }
inline int launch_bam_fill(const FqBamFillArgs &a) {      // (the variable is read at every call here, so that one test process holds either body to the texts)
  const char *form = getenv("FASTQUICK_BAM_FILL");
  if (form && !strcmp(form, "pieces")) { for (int e = 0; e < a.n_sides; ++e) for (uint64_t t = 0; t < fq_bam_fill_pieces(a, e); ++t) fq_bam_fill_piece(a, e, t); return 0; }
  for (uint32_t u = 0; u < a.n_units; ++u) for (int e = 0; e < a.n_sides; ++e) for (uint32_t lane = 0; lane < 64; ++lane) fq_bam_fill_lane(a, u, e, lane);
  return 0;
}
inline int bam_hash_bits() { const char *e = getenv("FASTQUICK_BAM_HASH_BITS"); const int v = e && *e ? atoi(e) : FQC_HASH_BITS; return v < 0 ? 0 : v > 64 ? 64 : v; }      // (read at every call here, as FASTQUICK_BAM_FILL)
inline int launch_bam_ckeys(const FqBamCollateArgs &a) { for (uint32_t c = 0; c < a.n; ++c) *a.bad = fqb_min64(*a.bad, fq_bam_ckey_thread(a, c)); return 0; }
inline int launch_bam_cmatch(const FqBamCollateArgs &a) { for (uint32_t i = 0; i < a.n; ++i) *a.bad = fqb_min64(*a.bad, fq_bam_cmatch_thread(a, i)); return 0; }
inline int launch_bam_cunits(const FqBamCollateArgs &a) { for (uint32_t k = 0; k < a.n_kept; ++k) fq_bam_cunit_thread(a, k); return 0; }
inline int launch_bam_cmark(const FqBamCollateArgs &a) { for (uint32_t c = 0; c < a.n; ++c) fq_bam_cmark_thread(a, c); return 0; }
inline int launch_bam_chold(const FqBamCollateArgs &a) { for (uint32_t c = 0; c < a.n; ++c) for (uint32_t lane = 0; lane < 64; ++lane) fq_bam_chold_lane(a, c, lane); return 0; }
#endif
}  // namespace fqdev
