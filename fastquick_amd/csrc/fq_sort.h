// fq_sort.h -- the coordinate order of BAM records, for the sorted writer (fq_bam.cpp: fq_bam_create_sorted): what the pipeline's `samtools sort` step
// (bin/FASTQuick_template.sh:501-502) does to O.bam, as a stable LSD radix sort of (key, ordinal) pairs with 8-bit digits.  The key is fq_emit.h's
// fq_bam_sort_key; the per-item bodies below -- a key's digit, a record's sort entry, a destination piece of the gather -- are stated once: fq_device.hip
// wraps them in kernels, and a build without hipcc (tests/emu) gets the three launchers as host loops over the same bodies, defined inline here.
//
//   a pass       per workgroup (FQ_SORT_TILE keys) a histogram of the pass's digit -> ONE scan over hist[digit][tile] -> scatter.  Inside a workgroup
//                the scatter takes 256 keys a round: a wavefront ranks equal digits in lane order with a ballot match (eight ballots), the four
//                wavefronts' counts meet in LDS, and the workgroup's running base per digit moves on.  No atomic decides a place: the result is THE
//                stable permutation on every run.
//   passes       only over the key_bits that can be set (a human reference: 34 bits, five passes)
#pragma once
#include <stdint.h>

#include "fq_emit.h"

#define FQ_SORT_DIGITS 256u
#define FQ_SORT_TILE 4096u            // keys of a workgroup in a pass: sixteen rounds of 256
// timing ids behind the public FQ_K_* (fqdev::time_collect with FQ_KX_COUNT ids): the entries, the sort's passes and the permutation; the gather.  Whoever collects them
// adds both to FQ_K_EMIT as well, which stays the time of all the consumers' kernels.
enum { FQ_KX_SORT = FQ_K_COUNT, FQ_KX_GATHER = FQ_K_COUNT + 1, FQ_KX_COUNT = FQ_K_COUNT + 2 };

struct FqBamSortEnt { uint64_t key; uint32_t len; int32_t end; };      // a record's key, its bytes (block_size included) and the end of its alignment on the reference
// the caller's ping-pong buffers: n keys, n ordinals, FQ_SORT_DIGITS x tiles counts (+ 1), as many offsets (+ 2)
struct FqSortScratch { uint64_t *key_tmp; uint32_t *perm_tmp; uint32_t *hist; uint64_t *hoff; };
struct FqBamKeyArgs { const uint8_t *rec; const uint64_t *off; const uint32_t *len; FqBamSortEnt *ent; uint64_t *key; uint32_t n; int32_t n_ref, pos_bits; };      // key: the entries' keys once more, as the sort's input
// records src[src_off[perm[i]] ...) to dst[dst_off[i] ...), i < n; dst_off[n] = total
struct FqBamGatherArgs { const uint8_t *src; const uint64_t *src_off; const uint32_t *perm; const uint64_t *dst_off; uint8_t *dst; uint32_t n; uint64_t total; };

FQ_HD int fq_sort_passes(int key_bits) { return key_bits <= 8 ? 1 : key_bits >= 64 ? 8 : (key_bits + 7) >> 3; }
FQ_HD uint32_t fq_sort_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + FQ_SORT_TILE - 1) / FQ_SORT_TILE); }
FQ_HD uint32_t fq_sort_digit(uint64_t key, int pass) { return (uint32_t)(key >> (8 * pass)) & 0xffu; }

FQ_HD uint32_t fq_sort_ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
FQ_HD uint32_t fq_sort_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// the sort entry of the record at r (block_size first; len bytes in all): refID, pos, flag at their fixed places, the CIGAR walked for the reference length
FQ_HD FqBamSortEnt fq_bam_sort_entry(const uint8_t *r, uint32_t len, int32_t n_ref, int32_t pos_bits) {
  FqBamSortEnt e;
  e.len = len;
  if (len < 36) { e.key = fq_bam_sort_key((uint32_t)n_ref, -1, 0, pos_bits); e.end = 0; return e; }      // (not a record: behind everything)
  const int32_t tid = (int32_t)fq_sort_ld32(r + 4), pos = (int32_t)fq_sort_ld32(r + 8);
  const uint32_t l_name = r[12], n_cig = fq_sort_ld16(r + 16), flag = fq_sort_ld16(r + 18);
  e.key = fq_bam_sort_key(tid < 0 ? (uint32_t)n_ref : (uint32_t)tid, pos, (int)(flag >> 4 & 1), pos_bits);
  int64_t rlen = 0;
  const uint8_t *cg = r + 36 + l_name;
  for (uint32_t k = 0; k < n_cig && 36 + l_name + 4 * (k + 1) <= len; ++k) {
    const uint32_t c = fq_sort_ld32(cg + 4 * k), op = c & 15;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;      // M D N = X
  }
  e.end = (flag & 4) || rlen == 0 ? pos + 1 : (int32_t)(pos + rlen);
  return e;
}
FQ_HD void fq_bam_key_thread(const FqBamKeyArgs &a, uint32_t i) {
  const FqBamSortEnt e = fq_bam_sort_entry(a.rec + a.off[i], a.len[i], a.n_ref, a.pos_bits);
  a.ent[i] = e; a.key[i] = e.key;
}
// sixteen destination bytes: the record that holds the first of them by bisection, then on through the records
FQ_HD void fq_bam_gather_piece(const FqBamGatherArgs &a, uint64_t t) {
  uint64_t b = t * 16;
  const uint64_t hi = b + 16 < a.total ? b + 16 : a.total;
  if (b >= hi) return;
  uint32_t lo = 0, up = a.n;                  // the last record with dst_off <= b
  while (up - lo > 1) { const uint32_t m = lo + ((up - lo) >> 1); if (a.dst_off[m] <= b) lo = m; else up = m; }
  uint32_t r = lo;
  while (b < hi) {
    while (r + 1 < a.n && a.dst_off[r + 1] <= b) ++r;
    const uint64_t rend = a.dst_off[r + 1] < hi ? a.dst_off[r + 1] : hi;
    const uint8_t *s = a.src + a.src_off[a.perm[r]] + (b - a.dst_off[r]);
    for (; b < rend; ++b) a.dst[b] = *s++;
    if (r + 1 >= a.n) break;
  }
}
// the same sixteen bytes gathered into four words and stored as words (dst is aligned to sixteen bytes): a whole piece, b + 16 <= total
FQ_HD void fq_bam_gather_piece16(const FqBamGatherArgs &a, uint64_t t) {
  uint64_t b = t * 16;
  const uint64_t hi = b + 16;
  uint32_t lo = 0, up = a.n;
  while (up - lo > 1) { const uint32_t m = lo + ((up - lo) >> 1); if (a.dst_off[m] <= b) lo = m; else up = m; }
  uint32_t r = lo, w[4] = {0, 0, 0, 0};
  while (b < hi) {
    while (r + 1 < a.n && a.dst_off[r + 1] <= b) ++r;
    const uint64_t rend = a.dst_off[r + 1] < hi ? a.dst_off[r + 1] : hi;
    const uint8_t *s = a.src + a.src_off[a.perm[r]] + (b - a.dst_off[r]);
    for (; b < rend; ++b) { const uint32_t k = (uint32_t)(b & 15); w[k >> 2] |= (uint32_t)*s++ << (8 * (k & 3)); }
    if (r + 1 >= a.n) break;
  }
  uint32_t *d = (uint32_t *)(a.dst + t * 16);
  d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3];
}
// a wavefront per record (lane of 64): the record's bytes, sixty-four at a time
FQ_HD void fq_bam_gather_record_lane(const FqBamGatherArgs &a, uint32_t i, uint32_t lane) {
  const uint64_t d0 = a.dst_off[i], len = a.dst_off[i + 1] - d0;
  const uint8_t *s = a.src + a.src_off[a.perm[i]];
  for (uint64_t k = lane; k < len; k += 64) a.dst[d0 + k] = s[k];
}

namespace fqdev {
// key_out / perm_out: the keys in stable ascending order and, for each, its place in key_in.  n < 2^32; nothing is waited for.
#if defined(__HIPCC__)
int launch_sort_pairs(const uint64_t *key_in, uint32_t n, int key_bits, uint64_t *key_out, uint32_t *perm_out, const FqSortScratch &s);
int launch_bam_key(const FqBamKeyArgs &a);                       // a thread per record
// ent_out[i] = ent[perm[i]] and len_out[i] = its length (the caller scans them into dst_off)
int launch_sort_permute(const FqBamSortEnt *ent, const uint32_t *perm, uint32_t n, FqBamSortEnt *ent_out, uint32_t *len_out);
int launch_bam_gather(const FqBamGatherArgs &a);                 // a wavefront per record (FASTQUICK_BAM_GATHER=pieces: a thread per sixteen destination bytes, A/B)
#else
// the host-loop tier: the same bodies, each pass ranked by a plain counting sort
inline int launch_sort_pairs(const uint64_t *key_in, uint32_t n, int key_bits, uint64_t *key_out, uint32_t *perm_out, const FqSortScratch &s) {
  if (!n) return 0;
  const int P = fq_sort_passes(key_bits);
  const uint64_t *kin = key_in;
  const uint32_t *pin = nullptr;
  for (int p = 0; p < P; ++p) {
    const bool to_out = ((P - 1 - p) & 1) == 0;
    uint64_t *ko = to_out ? key_out : s.key_tmp;
    uint32_t *po = to_out ? perm_out : s.perm_tmp;
    uint64_t at[FQ_SORT_DIGITS + 1] = {0};
    for (uint32_t i = 0; i < n; ++i) ++at[fq_sort_digit(kin[i], p) + 1];
    for (uint32_t d = 0; d < FQ_SORT_DIGITS; ++d) at[d + 1] += at[d];
    for (uint32_t i = 0; i < n; ++i) { const uint64_t w = at[fq_sort_digit(kin[i], p)]++; ko[w] = kin[i]; po[w] = pin ? pin[i] : i; }
    kin = ko; pin = po;
  }
  return 0;
}
inline int launch_bam_key(const FqBamKeyArgs &a) { for (uint32_t i = 0; i < a.n; ++i) fq_bam_key_thread(a, i); return 0; }
inline int launch_sort_permute(const FqBamSortEnt *ent, const uint32_t *perm, uint32_t n, FqBamSortEnt *ent_out, uint32_t *len_out) {
  for (uint32_t i = 0; i < n; ++i) { ent_out[i] = ent[perm[i]]; len_out[i] = ent_out[i].len; }
  return 0;
}
inline int launch_bam_gather(const FqBamGatherArgs &a) {      // (both forms in turn, so that either body is held to the files: the second overwrites the first's bytes with the same)
  for (uint64_t t = 0; t < (a.total + 15) / 16; ++t) { if (t * 16 + 16 <= a.total) fq_bam_gather_piece16(a, t); else fq_bam_gather_piece(a, t); }
  for (uint32_t i = 0; i < a.n; ++i) for (uint32_t lane = 0; lane < 64; ++lane) fq_bam_gather_record_lane(a, i, lane);
  return 0;
}
#endif
}  // namespace fqdev
