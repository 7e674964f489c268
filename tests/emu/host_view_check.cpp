// TEST INFRASTRUCTURE ONLY: the host formatters' view of a call (csrc/fq_align.cpp: fq_ctx_host_view -- the gather of qualities and names, the decode of a packed
// batch's surviving rows) under AddressSanitizer / UBSan, linked against the host-loop build of the library.  Aligns a FASTQ pair in batches from an ASCII batch and
// from a packed batch, with rows, names and qualities in heap blocks of exactly their size (stride = the longest read; an N every 41st base of every third read, so that
// the exception list is there), formats SAM text and BAM records on the host after every call and holds the packed side's bytes to the ASCII side's.  Each side also
// feeds a QC consumer of its own on the host (fq_qc_add_last without fq_ctx_attach_qc: the loop over fq_emit.h's StatCollector statement, which reads the rows through
// fq_emit_row and the view's strides); at the end the 13 files of the packed side must be the ASCII side's.  The index prefix is also the prefix of the QC inputs
// (.SelectedSite.vcf, .gc, .dbSNP.subset.vcf); the QC files go to a directory of their own under /tmp and are removed.
//     host_view_check <index prefix> <reads_1.fq> <reads_2.fq> <genome.fai> <batch pairs> <trim_qual>
// Exit code 0 and "ok" when nothing differs (and the sanitizers found nothing).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include <unistd.h>

#include "fastquick_amd.h"

struct Fastq { std::vector<std::string> name, seq, qual; };
static Fastq read_fastq(const char *path) {
  Fastq f;
  std::ifstream in(path);
  std::string a, b, c, d;
  while (std::getline(in, a) && std::getline(in, b) && std::getline(in, c) && std::getline(in, d)) { f.name.push_back(a.substr(1, a.find_first_of(" \t") - 1)); f.seq.push_back(b); f.qual.push_back(d); }
  return f;
}
#define MUST(x) do { if (x) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
static const char *const kQcFiles[13] = {"InsertSizeTable", "DepthDist", "GCDist", "EmpRepDist", "EmpCycleDist", "RawInsertSizeDist", "SexChromInfo", "Pileup",
                                         "FASTQ.csv", "Sequence.csv", "Summary", "AdjustedInsertSizeDist", "vcf"};
static std::string slurp(const std::string &path) {      // (the .vcf without the line that carries the day it was written)
  std::ifstream in(path, std::ios_base::binary);
  std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const size_t at = all.find("##fileDate=");
  if (at != std::string::npos) all.erase(at, all.find('\n', at) - at);
  return all;
}

int main(int argc, char **argv) {
  if (argc != 7) { fprintf(stderr, "usage: host_view_check <index prefix> <reads_1.fq> <reads_2.fq> <genome.fai> <batch pairs> <trim_qual>\n"); return 2; }
  Fastq fq[2] = {read_fastq(argv[2]), read_fastq(argv[3])};
  const int n = (int)fq[0].seq.size(), B = atoi(argv[5]);
  if (!n || fq[1].seq.size() != (size_t)n) { fprintf(stderr, "no reads\n"); return 2; }
  fq_index_t *ix = nullptr;
  MUST(fq_index_load(argv[1], 0, &ix));
  fq_opts_t o;
  fq_default_opts(&o);
  o.trim_qual = atoi(argv[6]);
  fq_qc_opts_t qo;
  fq_qc_default_opts(&qo);
  qo.genome_size = 3000000;
  fq_ctx_t *cx[2];
  fq_bam_t *bam[2];
  fq_qc_t *qc[2];
  char tmpl[] = "/tmp/host_view_check.XXXXXX";
  if (!mkdtemp(tmpl)) { fprintf(stderr, "no directory for the QC files\n"); return 1; }
  const std::string qc_out[2] = {std::string(tmpl) + "/ascii", std::string(tmpl) + "/packed"};
  for (int k = 0; k < 2; ++k) {
    MUST(fq_ctx_create(ix, &o, B, &cx[k])); MUST(fq_bam_create(ix, argv[4], nullptr, "@RG\tID:grp\tSM:s", &qo, &bam[k]));
    MUST(fq_qc_create(ix, argv[1], qc_out[k].c_str(), &qo, &qc[k])); MUST(fq_qc_begin_file(qc[k], argv[2], argv[3]));
  }
  long bad = 0, sam_bytes = 0, bam_bytes = 0;
  for (int b0 = 0; b0 < n; b0 += B) {
    const int m = std::min(B, n - b0);
    size_t stride = 1, ns = 1;
    for (int e = 0; e < 2; ++e) for (int i = 0; i < m; ++i) { stride = std::max(stride, fq[e].seq[b0 + i].size()); ns = std::max(ns, fq[0].name[b0 + i].size() + 1); }
    std::vector<uint8_t> seq(2 * (size_t)m * stride, 0), qual(2 * (size_t)m * stride, 0);
    std::vector<int32_t> len(2 * (size_t)m);
    std::vector<char> names((size_t)m * ns, 0);
    for (int e = 0; e < 2; ++e)
      for (int i = 0; i < m; ++i) {
        const std::string &s = fq[e].seq[b0 + i], &q = fq[e].qual[b0 + i];
        uint8_t *row = seq.data() + ((size_t)e * m + i) * stride;
        memcpy(row, s.data(), s.size());
        if ((b0 + i) % 3 == 0) for (size_t j = 40; j < s.size(); j += 41) row[j] = 'N';
        memcpy(qual.data() + ((size_t)e * m + i) * stride, q.data(), q.size());
        len[(size_t)e * m + i] = (int32_t)s.size();
        if (!e) memcpy(names.data() + (size_t)i * ns, fq[0].name[b0 + i].data(), fq[0].name[b0 + i].size());
      }
    fq_read_batch_t rb{m, (int32_t)stride, seq.data(), qual.data(), len.data(), names.data(), (int32_t)ns, nullptr};
    fq_packed_batch_t *pk = nullptr;
    MUST(fq_pack_reads(&rb, 2, &pk));
    fq_result_batch_t res[2];
    MUST(fq_align_batch(cx[0], &rb, &res[0]));
    MUST(fq_align_packed(cx[1], pk, &res[1]));
    std::vector<char> sam[2];
    const void *rec[2]; int64_t rec_len[2];
    for (int k = 0; k < 2; ++k) {
      const int64_t sz = fq_sam_format_last(cx[k], nullptr, 0);
      if (sz < 0) { fprintf(stderr, "fq_sam_format_last: %s\n", fq_ctx_last_error(cx[k])); return 1; }
      sam[k].resize((size_t)sz + 1);
      fq_sam_format_last(cx[k], sam[k].data(), sz + 1);
      MUST(fq_bam_format_last(bam[k], cx[k], &rec[k], &rec_len[k]));
      if (fq_qc_add_last(qc[k], cx[k])) { fprintf(stderr, "fq_qc_add_last: %s\n", fq_qc_last_error(qc[k])); return 1; }
    }
    if (sam[0] != sam[1]) { fprintf(stderr, "batch at %d: the packed batch's SAM text differs from the ASCII batch's\n", b0); ++bad; }
    if (rec_len[0] != rec_len[1] || memcmp(rec[0], rec[1], (size_t)rec_len[0]) != 0) { fprintf(stderr, "batch at %d: the packed batch's BAM records differ from the ASCII batch's\n", b0); ++bad; }
    sam_bytes += (long)sam[0].size() - 1; bam_bytes += (long)rec_len[0];
    fq_packed_free(pk);
  }
  for (int k = 0; k < 2; ++k) { MUST(fq_qc_end_file(qc[k])); MUST(fq_qc_write(qc[k])); fq_qc_destroy(qc[k]); fq_bam_close(bam[k]); fq_ctx_destroy(cx[k]); }
  fq_index_destroy(ix);
  long qc_bytes = 0;
  for (const char *f : kQcFiles) {
    const std::string a = slurp(qc_out[0] + "." + f), p = slurp(qc_out[1] + "." + f);
    if (a != p) { fprintf(stderr, "QC file %s: the packed side's differs from the ASCII side's (%zu vs %zu bytes)\n", f, p.size(), a.size()); ++bad; }
    qc_bytes += (long)a.size();
    for (int k = 0; k < 2; ++k) unlink((qc_out[k] + "." + f).c_str());
  }
  rmdir(tmpl);
  if (bad || !sam_bytes || !bam_bytes || qc_bytes < 10000) { fprintf(stderr, "%ld differences (%ld bytes of SAM text, %ld of BAM records, %ld of QC files)\n", bad, sam_bytes, bam_bytes, qc_bytes); return 1; }
  printf("ok: %d pairs, %ld bytes of SAM text, %ld bytes of BAM records, %ld bytes of QC files\n", n, sam_bytes, bam_bytes, qc_bytes);
  return 0;
}
