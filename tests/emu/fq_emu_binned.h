// TEST INFRASTRUCTURE ONLY: the binned form of the packed filter (csrc/fq_kernels.h "the same filter, binned") as host loops over the routines the kernels
// of fq_device.hip call: count and offsets, bin, probe bucket by bucket, verdict.  Returns the number of inconsistencies it met (a bucket that did not
// receive the entries counted for it, a mask word the verdict did not leave zero): 0.
#pragma once
#include <cstdint>
#include <vector>

#include "fq_kernels.h"

inline long fq_emu_prep_packed_binned(const FqPrepPackedArgs &a) {
  long bad = 0;
  const int front = fq_filter_front(a.o.filter_thresh);
  std::vector<uint32_t> base(FQ_BIN_BUCKETS + 1, 0), cursor(FQ_BIN_BUCKETS), mask((size_t)a.n_reads, 0);
  std::vector<FqBinEntry> ent((size_t)a.n_reads * (size_t)front);
  uint64_t kmer[3];
  for (int r = 0; r < a.n_reads; ++r) {
    for (int ch = 0; ch < 3; ++ch) kmer[ch] = a.head[(size_t)ch * (size_t)a.n_reads + (size_t)r];
    for (int q = 0; q < front; ++q) ++base[fq_bin_pos(q, fq_filter_key(kmer, q)) + 1];
  }
  for (int p = 0; p < FQ_BIN_BUCKETS; ++p) { base[p + 1] += base[p]; cursor[p] = base[p]; }
  for (int r = 0; r < a.n_reads; ++r) {
    for (int ch = 0; ch < 3; ++ch) kmer[ch] = a.head[(size_t)ch * (size_t)a.n_reads + (size_t)r];
    for (int q = 0; q < front; ++q) { const uint32_t key = fq_filter_key(kmer, q); ent[cursor[fq_bin_pos(q, key)]++] = fq_bin_entry(key, r, q); }
  }
  for (int p = 0; p < FQ_BIN_BUCKETS; ++p) {
    if (cursor[p] != base[p + 1]) ++bad;
    const uint8_t *region = fq_bin_region(a.ix, p);
    for (uint32_t i = base[p]; i < base[p + 1]; ++i) if (fq_bin_hit(region, ent[i])) mask[(size_t)fq_bin_read(ent[i])] |= fq_bin_mask_bit(ent[i]);
  }
  for (int r = 0; r < a.n_reads; ++r) fq_prep_binned_verdict_thread(a, mask.data(), r);
  for (int r = 0; r < a.n_reads; ++r) if (mask[(size_t)r]) ++bad;
  return bad;
}
