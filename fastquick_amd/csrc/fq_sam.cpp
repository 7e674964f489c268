// fq_sam.cpp -- the host side of the SAM consumer: the --sam_out text of the last call as a loop over fq_emit.h's fq_sam_line (bwa_print_sam1,
// libbwa/bwase.c:455-581 -- the routine the consumers' kernels run) on the host's view of the call, the header (bwase.c:593-599 +
// bwase.h:27-30), and the canonical per-stage dump used by the parity tests (same text as oracle/ref_driver.cpp).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fastquick_amd.h"
#include "fq_index.h"
#include "fq_kernels.h"
#include "fq_pipeline.h"

void fq_ctx_all_reads(const fq_ctx_t *c, const uint8_t **filtered, const int32_t **len_trim);

namespace {
struct Out {
  std::string s;
  void printf(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (n < (int)sizeof buf) s.append(buf, (size_t)n);
    else {
      std::vector<char> big((size_t)n + 1);
      va_start(ap, fmt);
      vsnprintf(big.data(), big.size(), fmt, ap);
      va_end(ap);
      s.append(big.data(), (size_t)n);
    }
  }
  void putc(char ch) { s.push_back(ch); }
};
int64_t emit(const std::string &s, char *buf, int64_t cap) {
  if (buf && cap > (int64_t)s.size()) { memcpy(buf, s.data(), s.size()); buf[s.size()] = 0; }
  return (int64_t)s.size();
}
void put_cigar(Out &o, const std::vector<uint16_t> &cg) { for (uint16_t x : cg) o.printf("%d%c", x & 0x3fff, "MIDS"[x >> 14]); }

void dump_cigar(Out &o, const std::vector<uint16_t> &cg) { if (cg.empty()) o.putc('*'); else put_cigar(o, cg); }
void dump_rec(Out &o, char tag, int end, int idx, const FqRead &p, bool fin) {
  o.printf("%c %d %d type=%d strand=%d pos=%u sa=%u mapQ=%d seQ=%d c1=%d c2=%d flag=%d mm=%d go=%d ge=%d score=%d filt=%d len=%d", tag, end, idx,
           p.type, p.strand, p.pos, p.sa, p.mapQ, p.seQ, (int)p.c1, (int)p.c2, p.extra_flag, p.n_mm, p.n_gapo, p.n_gape, p.score, p.filtered, p.len);
  o.s.append(" cigar=");
  dump_cigar(o, p.cigar);
  if (fin) o.printf(" nm=%d md=%s", p.nm, p.has_md ? p.md.c_str() : "*");
  o.printf(" multi=%d", (int)p.multi.size());
  for (const FqMulti &q : p.multi) { o.printf(" [%u,%d,%d,%d,", q.pos, q.gap, q.mm, q.strand); dump_cigar(o, q.cigar); o.putc(']'); }
  o.putc('\n');
}
}  // namespace

extern "C" int64_t fq_sam_header(const fq_index_t *ix, char *buf, int64_t cap) {
  if (!ix) return FQ_EINVAL;
  Out o;
  for (const auto &cg : ix->contigs) o.printf("@SQ\tSN:%s\tLN:%d\n", cg.name.c_str(), cg.len);
  o.s.append("@PG\tID:FastqA\tPN:FastqA\tVN:0.0.1\n");
  return emit(o.s, buf, cap);
}

// a thread per record measures its line, a prefix sum places the lines, a thread per record writes its line: emit_measure / emit_fill on the host
extern "C" int64_t fq_sam_format_last(fq_ctx_t *c, char *buf, int64_t cap) {
  if (!c) return FQ_EINVAL;
  FqSamArgs A;
  if (fq_ctx_host_view(c, &A)) return FQ_EINVAL;     // (no result arrays on the host: FQ_EMIT_DEVICE_ONLY -- fq_sam_device_last has the text)
  const size_t N = 2 * (size_t)A.n_surv;
  std::vector<uint32_t> len(N + 1), meta(N + 1);
  std::vector<uint64_t> off(N + 1);
  A.len = len.data(); A.meta = meta.data(); A.off = off.data(); A.text = buf; A.split = 0;
  fq_host_records(A.n_surv, [&](int idx) { fq_sam_len_thread(A, idx); });
  uint64_t total = 0;
  for (size_t i = 0; i < N; ++i) { off[i] = total; total += len[i]; }
  if (buf && cap > (int64_t)total) { fq_host_records(A.n_surv, [&](int idx) { fq_sam_fill_thread(A, idx); }); buf[total] = 0; }
  return (int64_t)total;
}

extern "C" int64_t fq_stage_dump_last(fq_ctx_t *c, char *buf, int64_t cap) {
  if (!c) return FQ_EINVAL;
  const FqBatchState *S = fq_ctx_state(c);
  const FqHostReads hbv = fq_ctx_host_reads(c), *hb = &hbv;
  const uint8_t *filt; const int32_t *ltrim;
  fq_ctx_all_reads(c, &filt, &ltrim);
  if (S->n_pairs > 0 && (!filt || !ltrim)) return FQ_EINVAL;   // per-read arrays of the whole batch are only fetched in debug mode
  if (S->n_surv > 0 && !S->rec) return FQ_EINVAL;
  const int n = S->n_pairs;
  const fq_opts_t *opts = fq_ctx_opts(c);
  const int n_ends = opts->single_end ? 1 : 2;   // the single-end mapper's dump has one end, no insert-size line and no mate-rescue stage
  Out o;
  std::vector<int> surv_of(n, -1);
  for (int sp = 0; sp < S->n_surv; ++sp) surv_of[S->pair_idx[sp]] = sp;
  const int Bp = S->batch_pairs > 0 ? S->batch_pairs : n;
  const int n_sub = n ? (n + Bp - 1) / Bp : 0;
  for (int sb = 0; sb < n_sub; ++sb) {
    const int i0 = sb * Bp, i1 = std::min(n, i0 + Bp);
    o.printf("B %d %d\n", sb, i1 - i0);
    for (int e = 0; e < n_ends; ++e)
      for (int i = i0; i < i1; ++i) o.printf("F %d %d filt=%d len=%d clip=%d full=%d\n", e, i - i0, filt[e * n + i], ltrim[e * n + i], ltrim[e * n + i], hb->len((size_t)e * n + i));
    for (int e = 0; e < n_ends; ++e)
      for (int i = i0; i < i1; ++i) {
        const int sp = surv_of[i];
        const int s = sp < 0 ? -1 : S->s_of(2 * (size_t)sp + e);
        const int na = s < 0 ? 0 : (int)S->aln_n[s];
        o.printf("A %d %d n=%d", e, i - i0, na);
        for (int k = 0; k < na; ++k) {
          const FqAln &a = S->aln[S->aln_off[s] + k];
          o.printf(" %d,%d,%d,%d,%u,%u,%d", a.info & 0xff, (a.info >> 8) & 0xff, (a.info >> 16) & 0xff, (a.info >> 24) & 1, a.k, a.l, a.score);
        }
        o.putc('\n');
      }
    const fq_isize_t &ii = S->isize_sub[sb];
    uint64_t a, s, p;
    memcpy(&a, &ii.avg, 8); memcpy(&s, &ii.std, 8); memcpy(&p, &ii.ap_prior, 8);
    if (n_ends == 2)
      o.printf("I avg=%016llx std=%016llx ap=%016llx low=%u high=%u hb=%u\n", (unsigned long long)a, (unsigned long long)s, (unsigned long long)p,
               ii.low, ii.high, ii.high_bayesian);
    const std::vector<FqRead> *stages[3] = {&S->stage_P, &S->stage_S, nullptr};   // (the final records: from the C-ABI arrays)
    const char tags[3] = {'P', 'S', 'R'};
    for (int st = 0; st < 3; ++st) {
      if (stages[st] && stages[st]->size() != (size_t)S->n_surv * 2) continue;   // snapshots are only kept in debug mode
      if (n_ends == 1 && st == 1) continue;
      for (int e = 0; e < n_ends; ++e)
        for (int i = i0; i < i1; ++i) {
          const int sp = surv_of[i];
          if (sp >= 0) { dump_rec(o, tags[st], e, i - i0, stages[st] ? (*stages[st])[2 * (size_t)sp + e] : S->read(2 * (size_t)sp + e), st == 2); continue; }
          FqRead d;   // both mates filtered: untouched record (bwa_clean_read_seq state + flags of BwtMapper.cpp:749)
          d.filtered = 1; d.extra_flag = n_ends == 1 ? 0 : (1 | (e == 0 ? 64 : 128)); d.len = ltrim[e * n + i]; d.full_len = hb->len((size_t)e * n + i);
          if (st == 2 && d.len != d.full_len) {   // bwa_correct_trimmed touches every record
            d.cigar.push_back((uint16_t)(FQ_OP_M << 14 | d.len)); d.cigar.push_back((uint16_t)(FQ_OP_S << 14 | (d.full_len - d.len))); d.len = d.full_len;
          }
          dump_rec(o, tags[st], e, i - i0, d, st == 2);
        }
    }
  }
  return emit(o.s, buf, cap);
}
