// fq_deflate.h -- BGZF members written ON THE DEVICE: one wavefront compresses one block of the BAM record stream into a complete gzip member
// (SAM/BAM specification 4.1: BC extra field, raw DEFLATE payload, CRC-32, ISIZE).
//
// What it replaces: the reference hands every SamRecord to SamFile::WriteRecord, whose BGZF layer (htslib's bgzf_write, VerifyBamID/statgen/
// BgzfFileType.h) deflates 64 KiB blocks with zlib on the one thread that also aligns.  A BAM file is defined by what it inflates to; which valid
// DEFLATE stream carries a block is the writer's choice -- so the blocks are compressed where the records are formatted (fq_emit.h), and the host
// only appends members to the file.
//
// The stream of a block is ONE fixed-Huffman block (RFC 1951, 3.2.6) of greedy LZ77 tokens:
//   * 64 positions per step, a lane each: hash of the 4 bytes there -> the last position of an EARLIER step with that hash (16-bit table in LDS),
//     match length by comparing words;
//   * the greedy parse of the step is the only serial part: a uniform loop over its tokens (a token per iteration: one readlane of the match length at
//     the parse position), which also hands every token its bit offset;
//   * every chosen lane ORs its code (Huffman codes bit-reversed: DEFLATE packs them from the most significant bit) into a small LDS buffer, whole
//     bytes of which leave for HBM once per step.
// Blocks are FQD_BLOCK bytes of input, so that a block of nothing but 9-bit literals still fits a 64 KiB member.
//
// A second mode (fqd_member_dyn) chooses the block type per member: the same parse, kept as tokens while the literal / length and distance
// symbols are counted; code lengths from the counts (fqd_code_lengths); BTYPE = 10 where its exact cost, header included, is below the fixed
// code's for the same tokens, BTYPE = 01 otherwise -- so a member of that mode is never larger than the fixed encoding of its parse.
//
// Written in the wavefront idiom of fq_frontend.h (FQF_LANES: once per lane on the device, a loop over 64 lanes in the host-loop build).
#pragma once
#include "fq_frontend.h"

#define FQD_BLOCK 0xd000u          // input bytes per member: 53,248 x 9 / 8 + 27 < 65,536
#define FQD_SLOT 65536u            // staging bytes per member
#define FQD_HBITS 11              // 2,048 hash slots: 4 KB of LDS per wavefront (with 4,096 twelve wavefronts fit a CU, and the kernel is bound by the latency of a step's dependent loads)
#define FQD_MIN_MATCH 4
#define FQD_MAX_MATCH 258

struct FqdLds {
  union {
    uint16_t htab[1 << FQD_HBITS]; // position + 1 of the last occurrence of a hash (0: none)
    uint32_t crc_tab[1024];        // ... and, when the block is compressed, the CRC's slice tables in the same bytes
  };
  uint32_t obuf[96];               // the step's bits
};
struct FqDeflateArgs {
  const uint8_t *in; uint64_t n;   // the record stream
  uint8_t *stage;                  // [n_blocks][FQD_SLOT]
  uint32_t *bsize;                 // [n_blocks] bytes of member b
  const FqzCrcConst *crc;
  uint32_t n_blocks;
  uint8_t *tok = nullptr;          // (dynamic mode) [n_blocks][FQD_SLOT]: a block's tokens between its parse and its emission -- the pack's destination, idle until then
};
struct FqDeflatePackArgs { const uint8_t *stage; const uint32_t *bsize; const uint64_t *off; uint8_t *out; uint32_t n_blocks; };

FQ_HD uint32_t fqd_rev(uint32_t code, int len) { return FQF_BREV32(code) >> (32 - len); }
// (bits, nbits) of a literal in the fixed code
FQ_HD void fqd_literal(uint32_t b, uint64_t *bits, int *nbits) {
  if (b < 144) { *bits = fqd_rev(0x30 + b, 8); *nbits = 8; }
  else { *bits = fqd_rev(0x190 + (b - 144), 9); *nbits = 9; }
}
// the symbol of a match length (257..285), of a distance (0..29): its extra bits' count and value
FQ_HD void fqd_len_sym(uint32_t len, uint32_t *lcode, uint32_t *leb, uint32_t *lex) {
  const uint32_t l = len - 3;
  if (l < 8) { *lcode = 257 + l; *leb = 0; *lex = 0; }
  else if (len == 258) { *lcode = 285; *leb = 0; *lex = 0; }
  else { const int n = 31 - __builtin_clz(l); *leb = (uint32_t)n - 2; *lcode = 257 + 4 * *leb + 4 + ((l >> *leb) & 3); *lex = l & ((1u << *leb) - 1); }
}
FQ_HD void fqd_dist_sym(uint32_t dist, uint32_t *dcode, uint32_t *deb, uint32_t *dex) {
  const uint32_t d = dist - 1;
  if (d < 4) { *dcode = d; *deb = 0; *dex = 0; }
  else { const int n = 31 - __builtin_clz(d); *deb = (uint32_t)n - 1; *dcode = 2 * (uint32_t)n + ((d >> (n - 1)) & 1); *dex = d & ((1u << *deb) - 1); }
}
// ... of a match: length code + extra bits, distance code + extra bits
FQ_HD void fqd_match(uint32_t len, uint32_t dist, uint64_t *bits, int *nbits) {
  uint32_t lcode, leb, lex, dcode, deb, dex;
  fqd_len_sym(len, &lcode, &leb, &lex);
  fqd_dist_sym(dist, &dcode, &deb, &dex);
  uint64_t v; int nb;
  if (lcode < 280) { v = fqd_rev(lcode - 256, 7); nb = 7; }
  else { v = fqd_rev(0xC0 + (lcode - 280), 8); nb = 8; }
  v |= (uint64_t)lex << nb; nb += (int)leb;
  v |= (uint64_t)fqd_rev(dcode, 5) << nb; nb += 5;
  v |= (uint64_t)dex << nb; nb += (int)deb;
  *bits = v; *nbits = nb;
}
FQ_HD uint32_t fqd_load32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// A per-lane register handed to a helper: the register itself on the device, the array of 64 in the host-loop build
#if defined(__HIP_DEVICE_COMPILE__)
#define FQD_LREF(T, name) T &name
#define FQD_ATOMIC_ADD32(p, v) atomicAdd((unsigned *)(p), (unsigned)(v))
#define FQD_MEM_FENCE() __threadfence()      // what the wavefront's lanes stored to HBM is what any of them loads from here on
#else
#define FQD_LREF(T, name) T *name
#define FQD_ATOMIC_ADD32(p, v) (*(p) += (uint32_t)(v))
#define FQD_MEM_FENCE() do { } while (0)
#endif

// ---- the token choice of one step of 64 positions, for either mode: mlen / mdist of a lane are the match its position starts (0: none); returns the
//      positions that emit a token (a set position with mlen is that match, one without the literal there).  carry: positions at the head of the step
//      that the last match of the step before covers.
FQ_HD uint64_t fqd_parse_step(const uint8_t *in, uint32_t n, uint32_t base, uint16_t *htab, uint32_t *carry, FQD_LREF(uint32_t, mlen), FQD_LREF(uint32_t, mdist)) {
  FQF_LVAR(uint32_t, hsh);
  // ---- candidates of the step: the table holds positions of earlier steps only
  FQF_LANES
    const uint32_t i = base + (uint32_t)lane;
    uint32_t L = 0, dist = 0, h = 0xffffffffu;
    if (i + FQD_MIN_MATCH <= n) {
      const uint32_t v = fqd_load32(in + i);
      h = (v * 2654435761u) >> (32 - FQD_HBITS);
      const uint32_t c1 = htab[h];
      if (c1 && i - (c1 - 1) <= 32768u) {            // (DEFLATE's window)
        const uint32_t c = c1 - 1;
        if (fqd_load32(in + c) == v) {
          const uint32_t cap = n - i < FQD_MAX_MATCH ? n - i : FQD_MAX_MATCH;
          L = 4;
          while (L + 4 <= cap && fqd_load32(in + c + L) == fqd_load32(in + i + L)) L += 4;
          while (L < cap && in[c + L] == in[i + L]) ++L;
          dist = i - c;
        }
      }
    }
    FQF_LV(mlen) = L; FQF_LV(mdist) = dist; FQF_LV(hsh) = h;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    if (FQF_LV(hsh) != 0xffffffffu) htab[FQF_LV(hsh)] = (uint16_t)(base + (uint32_t)lane + 1);      // (several lanes, one slot: any of them is a valid candidate)
  FQF_LANES_END
  // ---- the greedy parse of the step.  Only matches make it serial: between two chosen matches every position is a literal, so the loop runs once
  //      per chosen MATCH (find the next candidate at or behind the parse position in the ballot of the lanes that found one; everything in front
  //      of it is literals) -- a handful of iterations per step on BAM records, where a token per iteration was sixty.
  const uint32_t step_n = n - base < 64 ? n - base : 64;
  uint64_t cand = 0;                         // lanes whose position starts a match
#if defined(__HIP_DEVICE_COMPILE__)
  cand = __ballot(mlen != 0);
#else
  for (int l = 0; l < 64; ++l) if (mlen[l]) cand |= 1ull << l;
#endif
  uint64_t chosen = 0;                       // positions that emit a token
  uint32_t pos = *carry;
  while (pos < step_n) {
    const uint64_t ahead = cand >> pos;
    if (!ahead) { chosen |= (~0ull >> (64 - step_n)) & (~0ull << pos); pos = step_n; break; }      // literals to the end of the step
    const uint32_t c = pos + (uint32_t)__builtin_ctzll(ahead);
    if (c >= step_n) { chosen |= (~0ull >> (64 - step_n)) & (~0ull << pos); pos = step_n; break; }
    if (c > pos) chosen |= (~0ull >> (64 - c)) & (~0ull << pos);      // literals in front of the match
    chosen |= 1ull << c;
    pos = c + FQF_RL(mlen, c);
  }
  *carry = pos - step_n;
  return chosen;
}
// ---- the chosen tokens' bits (at most 48 each) behind the *bit_in bits that wait in obuf: their offsets are a prefix sum over the chosen lanes; whole
//      bytes leave for HBM, the partial byte stays as the head of the next step's buffer
FQ_HD void fqd_put_step(uint32_t *obuf, uint8_t *out, uint64_t chosen, FQD_LREF(uint32_t, tok_lo), FQD_LREF(uint32_t, tok_hi), FQD_LREF(uint32_t, tok_nb), uint32_t *byte_base, uint32_t *bit_in) {
  FQF_LVAR(uint32_t, sel); FQF_LVAR(uint32_t, off);
  uint32_t bit = *bit_in;
#if defined(__HIP_DEVICE_COMPILE__)
  {
    const int lane = (int)(threadIdx.x & 63);
    sel = (uint32_t)((chosen >> lane) & 1ull);
    const uint32_t nb = sel ? tok_nb : 0u;
    uint32_t inc = nb;                       // inclusive prefix sum over the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= d) inc += up; }
    off = *bit_in + inc - nb;
    bit = *bit_in + (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  }
#else
  for (int l = 0; l < 64; ++l) { sel[l] = (uint32_t)((chosen >> l) & 1ull); off[l] = bit; if (sel[l]) bit += tok_nb[l]; }
#endif
  FQF_LANES
    if (FQF_LV(sel)) {
      const uint64_t v = (uint64_t)FQF_LV(tok_lo) | (uint64_t)FQF_LV(tok_hi) << 32;
      const uint32_t o = FQF_LV(off), w = o >> 5, s = o & 31;
      FQF_ATOMIC_OR32(&obuf[w], (uint32_t)(v << s));
      const uint64_t rest = s ? v >> (32 - s) : v >> 32;
      if ((uint32_t)rest) FQF_ATOMIC_OR32(&obuf[w + 1], (uint32_t)rest);
      if (rest >> 32) FQF_ATOMIC_OR32(&obuf[w + 2], (uint32_t)(rest >> 32));
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  const uint32_t full = bit >> 3;
  FQF_LANES
    for (uint32_t j = (uint32_t)lane; j < full; j += 64) out[*byte_base + j] = (uint8_t)(obuf[j >> 2] >> (8 * (j & 3)));
  FQF_LANES_END
  FQF_WAVE_FENCE();
  const uint32_t tail = (obuf[full >> 2] >> (8 * (full & 3))) & 0xffu;
  FQF_WAVE_FENCE();
  FQF_LANES
    for (int i = lane; i < 96; i += 64) obuf[i] = i == 0 ? tail : 0u;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  *byte_base += full; *bit_in = bit & 7;
}
// ---- the member's end: the last byte of the block (the end-of-block code is in obuf, *bit_in counts it), then the gzip header with BSIZE, CRC-32 and
//      ISIZE.  Returns the member's size.
FQ_HD uint32_t fqd_finish(const FqDeflateArgs &A, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t *obuf, uint32_t *crc_tab, uint32_t byte_base, uint32_t bit_in) {
  const uint32_t last = (bit_in + 7) >> 3;
  FQF_LANES
    for (uint32_t j = (uint32_t)lane; j < last; j += 64) out[byte_base + j] = (uint8_t)(obuf[j >> 2] >> (8 * (j & 3)));
  FQF_LANES_END
  byte_base += last;
  const uint32_t crc = fqz_crc_wave(in, n, A.crc, crc_tab);
  const uint32_t bs = byte_base + 8;
  FQF_LANES
    if (lane == 0) {
      const uint8_t hdr[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)((bs - 1) & 0xff), (uint8_t)((bs - 1) >> 8)};
      for (int k = 0; k < 18; ++k) out[k] = hdr[k];
      for (int k = 0; k < 4; ++k) { out[byte_base + k] = (uint8_t)(crc >> (8 * k)); out[byte_base + 4 + k] = (uint8_t)(n >> (8 * k)); }
    }
  FQF_LANES_END
  return bs;
}

// member b of the record stream: returns its size (header and trailer included)
FQ_HD uint32_t fqd_member(const FqDeflateArgs &A, uint32_t b, FqdLds &S) {
  const uint64_t lo = (uint64_t)b * FQD_BLOCK;
  const uint32_t n = (uint32_t)(A.n - lo < FQD_BLOCK ? A.n - lo : FQD_BLOCK);
  const uint8_t *in = A.in + lo;
  uint8_t *out = A.stage + (size_t)b * FQD_SLOT;
  FQF_LANES
    for (int i = lane; i < (1 << FQD_HBITS); i += 64) S.htab[i] = 0;
    for (int i = lane; i < 96; i += 64) S.obuf[i] = 0;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  // the block header: BFINAL = 1, BTYPE = 01 (fixed Huffman) -- bits 1, 1, 0
  uint32_t byte_base = 18, bit_in = 3;
  FQF_LANES
    if (lane == 0) S.obuf[0] = 3;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LVAR(uint32_t, mlen); FQF_LVAR(uint32_t, mdist); FQF_LVAR(uint32_t, tok_lo); FQF_LVAR(uint32_t, tok_hi); FQF_LVAR(uint32_t, tok_nb);
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint64_t chosen = fqd_parse_step(in, n, base, S.htab, &carry, mlen, mdist);
    FQF_LANES
      const uint32_t i = base + (uint32_t)lane;
      uint64_t bits; int nb;
      if (FQF_LV(mlen)) fqd_match(FQF_LV(mlen), FQF_LV(mdist), &bits, &nb);
      else if (i < n) fqd_literal(in[i], &bits, &nb);
      else { bits = 0; nb = 0; }
      FQF_LV(tok_lo) = (uint32_t)bits; FQF_LV(tok_hi) = (uint32_t)(bits >> 32); FQF_LV(tok_nb) = (uint32_t)nb;
    FQF_LANES_END
    fqd_put_step(S.obuf, out, chosen, tok_lo, tok_hi, tok_nb, &byte_base, &bit_in);
  }
  // end of block (symbol 256: seven zero bits)
  return fqd_finish(A, in, n, out, S.obuf, S.crc_tab, byte_base, bit_in + 7);
}
// members packed behind each other: thread t copies 16 bytes of member b = t / (FQD_SLOT / 16)
FQ_HD void fqd_pack_piece(const FqDeflatePackArgs &A, uint64_t t) {
  const uint32_t b = (uint32_t)(t / (FQD_SLOT / 16)), k = (uint32_t)(t % (FQD_SLOT / 16)) * 16;
  if (b >= A.n_blocks || k >= A.bsize[b]) return;
  const uint8_t *src = A.stage + (size_t)b * FQD_SLOT + k;
  uint8_t *dst = A.out + A.off[b] + k;
  const uint32_t m = A.bsize[b] - k < 16 ? A.bsize[b] - k : 16;
  for (uint32_t j = 0; j < m; ++j) dst[j] = src[j];
}

// =====================================================================================================================================
// Dynamic mode: the block type chosen per member
// =====================================================================================================================================
#define FQD_MAX_SYMS 288
struct FqdHuff {                   // what fqd_code_lengths works in
  uint32_t f[FQD_MAX_SYMS];        // the frequencies the code is made for (the two-codes rule applied)
  uint32_t nf[FQD_MAX_SYMS];       // the internal nodes' frequencies, in the order they are made
  uint16_t srt[FQD_MAX_SYMS];      // the used symbols by (frequency, symbol)
  uint16_t par[2 * FQD_MAX_SYMS];  // the parent of a node: the leaves in sorted order, the internal nodes behind them
  uint32_t blc[16];                // codes per length
  uint32_t used;
};
// Code lengths of a complete prefix code over the symbols with freq != 0, none longer than limit: Huffman's lengths where those fit.  Like zlib, never
// fewer than two codes: with one symbol used, or none, symbols of frequency 0 get the missing one-bit codes.  By one wavefront: the symbols ranked by
// (frequency, symbol) across the lanes, the two-queue merge by one lane (a leaf before an internal node of the same weight: the shallowest of the
// optimal trees), the leaves' depths by the lanes.  Beyond the limit the depths are clipped and the counts per length repaired one unit of the Kraft sum
// at a time (a code leaves the limit's row, the deepest code above it moves one row down and takes that code as its sibling); the lengths then go to
// the symbols by rank, the longest to the rarest.  Needs 2 <= n_sym <= FQD_MAX_SYMS, n_sym <= 2^limit, limit <= 15, the frequencies' sum below 2^32.
// halves: the frequencies are 16 bits wide, two to a word (fqd_count).
FQ_HD uint32_t fqd_count(const uint32_t *freq, int s) { return freq[s >> 1] >> (16 * (s & 1)) & 0xffffu; }
FQ_HD void fqd_code_lengths(const uint32_t *freq, int n_sym, int limit, uint8_t *len, FqdHuff &W, bool halves = false) {
  FQF_WAVE_FENCE();
  FQF_LANES
    for (int s = lane; s < n_sym; s += 64) { W.f[s] = halves ? fqd_count(freq, s) : freq[s]; len[s] = 0; }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    if (lane == 0) {
      uint32_t used = 0;
      int max_code = -1;
      for (int s = 0; s < n_sym; ++s) if (W.f[s]) { ++used; max_code = s; }
      while (used < 2) { const int s = max_code < 2 && max_code + 1 < n_sym ? ++max_code : 0; W.f[s] = 1; ++used; }
      W.used = used;
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  const uint32_t used = FQF_UNIFORM32(W.used);
  FQF_LANES
    for (int s = lane; s < n_sym; s += 64) {
      const uint32_t fs = W.f[s];
      if (!fs) continue;
      uint32_t r = 0;
      for (int t = 0; t < n_sym; ++t) { const uint32_t ft = W.f[t]; r += (ft != 0 && (ft < fs || (ft == fs && t < s))) ? 1u : 0u; }
      W.srt[r] = (uint16_t)s;
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    if (lane == 0) {
      uint32_t li = 0, ii = 0;                 // the next leaf, the next internal node: both queues ascend
      for (uint32_t made = 0; made + 1 < used; ++made) {
        uint32_t sum = 0;
        for (int k = 0; k < 2; ++k) {
          uint32_t node;
          if (li < used && (ii >= made || W.f[W.srt[li]] <= W.nf[ii])) { node = li; sum += W.f[W.srt[li]]; ++li; }
          else { node = used + ii; sum += W.nf[ii]; ++ii; }
          W.par[node] = (uint16_t)(used + made);
        }
        W.nf[made] = sum;
      }
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    for (uint32_t j = (uint32_t)lane; j < used; j += 64) {
      uint32_t d = 0;
      for (uint32_t node = j; node != 2 * used - 2; node = W.par[node]) ++d;
      len[W.srt[j]] = (uint8_t)(d < (uint32_t)limit ? d : (uint32_t)limit);
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    if (lane == 0) {
      for (int k = 0; k < 16; ++k) W.blc[k] = 0;
      for (uint32_t j = 0; j < used; ++j) ++W.blc[len[W.srt[j]]];
      uint32_t total = 0;                      // the Kraft sum in units of 2^-limit
      for (int k = 1; k <= limit; ++k) total += W.blc[k] << (limit - k);
      while (total > (1u << limit) && W.blc[limit]) {
        --W.blc[limit];
        for (int k = limit - 1; k > 0; --k) if (W.blc[k]) { --W.blc[k]; W.blc[k + 1] += 2; break; }
        --total;
      }
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    for (uint32_t j = (uint32_t)lane; j < used; j += 64) {
      uint32_t cum = 0;
      int k = limit;
      for (; k > 1; --k) { cum += W.blc[k]; if (j < cum) break; }
      len[W.srt[j]] = (uint8_t)k;
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
}
// (one lane) the canonical codes of the lengths (RFC 1951, 3.2.2), bit-reversed as the stream wants them; w: 16 words
FQ_HD void fqd_canon_codes(const uint8_t *len, int n, uint16_t *code, uint32_t *w) {
  for (int k = 0; k < 16; ++k) w[k] = 0;
  for (int s = 0; s < n; ++s) ++w[len[s]];
  uint32_t c = 0, prev = 0;
  for (int k = 1; k < 16; ++k) { c = (c + prev) << 1; prev = w[k]; w[k] = c; }
  for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)fqd_rev(w[len[s]]++, len[s]) : (uint16_t)0;
}
// the symbol of the code-length alphabet that begins at L[i] of the sequence L[0, n), and its extra bits; returns how many lengths it covers
FQ_HD int fqd_rle_next(const uint8_t *L, int n, int i, uint32_t *sym, uint32_t *ex, uint32_t *eb) {
  const uint32_t cur = L[i];
  int run = 1;
  while (i + run < n && L[i + run] == cur && run < 138) ++run;
  if (cur == 0 && run >= 11) { *sym = 18; *ex = (uint32_t)run - 11; *eb = 7; return run; }
  if (cur == 0 && run >= 3) { *sym = 17; *ex = (uint32_t)run - 3; *eb = 3; return run; }
  if (cur != 0 && i > 0 && L[i - 1] == cur && run >= 3) { if (run > 6) run = 6; *sym = 16; *ex = (uint32_t)run - 3; *eb = 2; return run; }
  *sym = cur; *ex = 0; *eb = 0;
  return 1;
}
// the i-th symbol in the order the code-length code's lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
FQ_HD uint32_t fqd_cl_order(int i) { return i < 3 ? 16u + (uint32_t)i : i == 3 ? 0u : (i & 1) ? 7u - (uint32_t)((i - 5) / 2) : 8u + (uint32_t)((i - 4) / 2); }
// (one lane) nb bits behind the *nacc waiting in *acc; whole bytes to out
FQ_HD void fqd_put_bits(uint8_t *out, uint32_t *pos, uint64_t *acc, uint32_t *nacc, uint32_t v, uint32_t nb) {
  *acc |= (uint64_t)v << *nacc; *nacc += nb;
  while (*nacc >= 8) { out[(*pos)++] = (uint8_t)*acc; *acc >>= 8; *nacc -= 8; }
}

struct FqdDynLds {
  union {
    uint16_t htab[1 << FQD_HBITS];   // the parse's table;
    FqdHuff huff;                    // ... then, in the same bytes, what the code lengths are made in;
    uint32_t crc_tab[1024];          // ... then the CRC's slice tables
  };
  union {
    uint32_t obuf[96];
    uint8_t seq[320];                // (before the first token's bits) the HLIT + HDIST lengths the header sends
  };
  union {
    uint32_t freq[160];              // the symbols' counts, 16 bits each (a block has fewer than 2^16 tokens), two to a word: literal / length at 0 (286 of them), distance at 288 (30);
    uint16_t code[320];              // ... then, in the same bytes, their codes, bit-reversed
  };
  uint8_t len[320];                  // the codes' lengths (the literal / length alphabet 288 wide and the distances 32, as the fixed code counts them)
  uint32_t clf[19];                  // the code-length code: counts, codes, lengths
  uint16_t clcode[19];
  uint8_t cll[19];
  uint32_t hv[5];                    // out of lane 0 for all: HLIT, HDIST, BTYPE, (bits waiting) << 16 | bytes of the header written, the bits waiting
};
// A block's tokens between its parse and its emission, in the block's slot of A.tok: a match's length - 3 and distance - 1 in the three bytes at the
// position it starts at (it covers four at least, so they are its own), and per step the 64 bits of the positions that emit a token behind the
// FQD_BLOCK bytes.  A literal is the input's byte; a token is a match exactly when the position behind it emits none.
FQ_HD uint32_t fqd_member_dyn(const FqDeflateArgs &A, uint32_t b, FqdDynLds &S) {
  const uint64_t lo = (uint64_t)b * FQD_BLOCK;
  const uint32_t n = (uint32_t)(A.n - lo < FQD_BLOCK ? A.n - lo : FQD_BLOCK);
  const uint8_t *in = A.in + lo;
  uint8_t *out = A.stage + (size_t)b * FQD_SLOT, *tok = A.tok + (size_t)b * FQD_SLOT;
  uint64_t *mask = (uint64_t *)(tok + FQD_BLOCK);
  FQF_LANES
    for (int i = lane; i < (1 << FQD_HBITS); i += 64) S.htab[i] = 0;
    for (int i = lane; i < 160; i += 64) S.freq[i] = 0;
    for (int i = lane; i < 320; i += 64) S.len[i] = 0;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  // ---- 1. the parse, once: the tokens kept, their symbols counted
  FQF_LVAR(uint32_t, mlen); FQF_LVAR(uint32_t, mdist); FQF_LVAR(uint32_t, tok_lo); FQF_LVAR(uint32_t, tok_hi); FQF_LVAR(uint32_t, tok_nb);
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint64_t chosen = fqd_parse_step(in, n, base, S.htab, &carry, mlen, mdist);
    FQF_LANES
      const uint32_t i = base + (uint32_t)lane;
      if ((chosen >> lane) & 1ull) {
        if (FQF_LV(mlen)) {
          uint32_t lcode, leb, lex, dcode, deb, dex;
          fqd_len_sym(FQF_LV(mlen), &lcode, &leb, &lex);
          fqd_dist_sym(FQF_LV(mdist), &dcode, &deb, &dex);
          const uint32_t d = FQF_LV(mdist) - 1;
          tok[i] = (uint8_t)(FQF_LV(mlen) - 3); tok[i + 1] = (uint8_t)d; tok[i + 2] = (uint8_t)(d >> 8);
          FQD_ATOMIC_ADD32(&S.freq[lcode >> 1], 1u << (16 * (lcode & 1))); FQD_ATOMIC_ADD32(&S.freq[144 + (dcode >> 1)], 1u << (16 * (dcode & 1)));
        } else FQD_ATOMIC_ADD32(&S.freq[in[i] >> 1], 1u << (16 * (in[i] & 1)));
      }
      if (lane == 0) mask[base >> 6] = chosen;
    FQF_LANES_END
  }
  FQF_LANES
    if (lane == 0) FQD_ATOMIC_ADD32(&S.freq[256 >> 1], 1);
  FQF_LANES_END
  FQD_MEM_FENCE();
  // ---- 2. the code lengths (the table of the parse is dead)
  fqd_code_lengths(S.freq, 286, 15, S.len, S.huff, true);
  fqd_code_lengths(S.freq + 144, 30, 15, S.len + 288, S.huff, true);
  // ---- 3. the header, and which block type costs fewer bits
  FQF_LANES
    if (lane == 0) {
      uint32_t hlit = 286, hdist = 30;
      while (hlit > 257 && !S.len[hlit - 1]) --hlit;
      while (hdist > 1 && !S.len[288 + hdist - 1]) --hdist;
      S.hv[0] = hlit; S.hv[1] = hdist;
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  const int hlit = (int)FQF_UNIFORM32(S.hv[0]), hdist = (int)FQF_UNIFORM32(S.hv[1]), n_seq = hlit + hdist;
  FQF_LANES
    for (int i = lane; i < n_seq; i += 64) S.seq[i] = i < hlit ? S.len[i] : S.len[288 + i - hlit];
    if (lane < 19) S.clf[lane] = 0;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  FQF_LANES
    if (lane == 0) {
      uint32_t sym, ex, eb;
      for (int i = 0; i < n_seq;) { i += fqd_rle_next(S.seq, n_seq, i, &sym, &ex, &eb); ++S.clf[sym]; }
    }
  FQF_LANES_END
  fqd_code_lengths(S.clf, 19, 7, S.cll, S.huff);
  FQF_LANES
    if (lane == 0) {
      int hclen = 19;
      while (hclen > 4 && !S.cll[fqd_cl_order(hclen - 1)]) --hclen;
      fqd_canon_codes(S.cll, 19, S.clcode, S.huff.blc);
      // the two costs without what they share (the three bits in front, the tokens' extra bits), and the three codes complete (the decoders ask for that)
      uint32_t dyn = 14 + 3 * (uint32_t)hclen + 2 * S.clf[16] + 3 * S.clf[17] + 7 * S.clf[18], fix = 0, kl = 0, kd = 0, kc = 0;
      for (int s = 0; s < 19; ++s) { dyn += S.clf[s] * S.cll[s]; if (S.cll[s]) kc += 1u << (7 - S.cll[s]); }
      for (int s = 0; s < 286; ++s) { const uint32_t f = fqd_count(S.freq, s); dyn += f * S.len[s]; fix += f * (s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u); if (S.len[s]) kl += 1u << (15 - S.len[s]); }
      for (int s = 0; s < 30; ++s) { const uint32_t f = fqd_count(S.freq, 288 + s); dyn += f * S.len[288 + s]; fix += f * 5u; if (S.len[288 + s]) kd += 1u << (15 - S.len[288 + s]); }
      const bool take = dyn < fix && kl == (1u << 15) && kd == (1u << 15) && kc == (1u << 7) && S.len[256];
      S.hv[2] = take ? 2u : 1u;
      uint32_t pos = 18, nacc = 0;
      uint64_t acc = 0;
      if (take) {     // BFINAL = 1, BTYPE = 10; HLIT, HDIST, HCLEN; the code-length code's lengths; the lengths, run-length coded across the two alphabets
        fqd_put_bits(out, &pos, &acc, &nacc, 5, 3);
        fqd_put_bits(out, &pos, &acc, &nacc, (uint32_t)hlit - 257, 5); fqd_put_bits(out, &pos, &acc, &nacc, (uint32_t)hdist - 1, 5); fqd_put_bits(out, &pos, &acc, &nacc, (uint32_t)hclen - 4, 4);
        for (int i = 0; i < hclen; ++i) fqd_put_bits(out, &pos, &acc, &nacc, S.cll[fqd_cl_order(i)], 3);
        uint32_t sym, ex, eb;
        for (int i = 0; i < n_seq;) {
          i += fqd_rle_next(S.seq, n_seq, i, &sym, &ex, &eb);
          fqd_put_bits(out, &pos, &acc, &nacc, S.clcode[sym], S.cll[sym]);
          if (eb) fqd_put_bits(out, &pos, &acc, &nacc, ex, eb);
        }
      } else fqd_put_bits(out, &pos, &acc, &nacc, 3, 3);      // BFINAL = 1, BTYPE = 01, as fqd_member
      S.hv[3] = nacc << 16 | (pos - 18); S.hv[4] = (uint32_t)acc;
    }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  const uint32_t head_bits = FQF_UNIFORM32(S.hv[4]);
  FQF_LANES
    for (int i = lane; i < 96; i += 64) S.obuf[i] = i == 0 ? head_bits : 0u;      // (the sequence is sent: its bytes are the tokens' buffer from here on)
  FQF_LANES_END
  FQF_WAVE_FENCE();
  const bool dynamic = FQF_UNIFORM32(S.hv[2]) == 2;
  uint32_t byte_base = 18 + (FQF_UNIFORM32(S.hv[3]) & 0xffffu), bit_in = FQF_UNIFORM32(S.hv[3]) >> 16;
  if (!dynamic) {     // the fixed code is the canonical code of these lengths
    FQF_LANES
      for (int s = lane; s < 320; s += 64) S.len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    FQF_LANES_END
    FQF_WAVE_FENCE();
  }
  FQF_LANES
    if (lane == 0) { fqd_canon_codes(S.len, 288, S.code, S.huff.blc); fqd_canon_codes(S.len + 288, 32, S.code + 288, S.huff.blc); }
  FQF_LANES_END
  FQF_WAVE_FENCE();
  // ---- 4. the kept tokens, 64 positions a step (a match covers four positions: seventeen matches of 48 bits at most and literals of 15, under half of obuf)
  for (uint32_t base = 0; base < n; base += 64) {
    const uint64_t chosen = mask[base >> 6], behind = base + 64 < n ? mask[(base >> 6) + 1] : 0ull;
    const uint64_t match = chosen & ~(chosen >> 1 | behind << 63);
    FQF_LANES
      const uint32_t i = base + (uint32_t)lane;
      uint64_t v = 0;
      uint32_t nb = 0;
      if ((chosen >> lane) & 1ull) {
        if (((match >> lane) & 1ull) && i + 1 < n) {
          uint32_t lcode, leb, lex, dcode, deb, dex;
          fqd_len_sym((uint32_t)tok[i] + 3, &lcode, &leb, &lex);
          fqd_dist_sym(((uint32_t)tok[i + 1] | (uint32_t)tok[i + 2] << 8) + 1, &dcode, &deb, &dex);
          v = S.code[lcode]; nb = S.len[lcode];
          v |= (uint64_t)lex << nb; nb += leb;
          v |= (uint64_t)S.code[288 + dcode] << nb; nb += S.len[288 + dcode];
          v |= (uint64_t)dex << nb; nb += deb;
        } else { v = S.code[in[i]]; nb = S.len[in[i]]; }
      }
      FQF_LV(tok_lo) = (uint32_t)v; FQF_LV(tok_hi) = (uint32_t)(v >> 32); FQF_LV(tok_nb) = nb;
    FQF_LANES_END
    fqd_put_step(S.obuf, out, chosen, tok_lo, tok_hi, tok_nb, &byte_base, &bit_in);
  }
  // end of block
  FQF_LANES
    if (lane == 0) S.obuf[0] |= (uint32_t)S.code[256] << bit_in;
  FQF_LANES_END
  FQF_WAVE_FENCE();
  bit_in += FQF_UNIFORM32(S.len[256]);
  FQF_WAVE_FENCE();
  return fqd_finish(A, in, n, out, S.obuf, S.crc_tab, byte_base, bit_in);
}

namespace fqdev {
// launch_deflate in dynamic mode (a.tok set), and fqd_code_lengths alone by one wavefront (tests): the same timing slot, the same stream
#if defined(__HIPCC__)
int launch_deflate_dyn(const FqDeflateArgs &a);
int launch_code_lengths(const uint32_t *freq, int n_sym, int limit, uint8_t *len);
#else
// the host-loop tier: the same bodies
inline int launch_deflate_dyn(const FqDeflateArgs &a) {
  static thread_local FqdDynLds lds;
  for (uint32_t b = 0; b < a.n_blocks; ++b) a.bsize[b] = fqd_member_dyn(a, b, lds);
  return 0;
}
inline int launch_code_lengths(const uint32_t *freq, int n_sym, int limit, uint8_t *len) {
  static thread_local FqdHuff w;
  fqd_code_lengths(freq, n_sym, limit, len, w);
  return 0;
}
#endif
}  // namespace fqdev
