// TEST INFRASTRUCTURE ONLY: the BGZF compressor's two modes (csrc/fq_deflate.h: fqd_member, fqd_member_dyn, fqd_code_lengths) under AddressSanitizer / UBSan, linked
// against the host-loop build of the library.  Every input goes through fq_bgzf_deflate_device (the old entry), fq_bgzf_deflate_device_mode(fixed) and (dynamic): the fixed
// mode's bytes must be the old entry's, every member must inflate with zlib to its block of the input with the right CRC-32 and ISIZE, and a dynamic member must not
// be larger than the fixed member of the same block.  fq_huffman_lengths_device is held to a complete prefix code within its limit that costs what Huffman's costs
// where Huffman's depth fits.  The inputs are made here (the kinds tests/test_deflate_dynamic.py uses, from a generator of this file).
//     deflate_dyn_check
// Exit code 0 and "ok" when nothing differs (and the sanitizers found nothing).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <queue>
#include <string>
#include <unordered_set>
#include <vector>
#include <zlib.h>

#include "fastquick_amd.h"

static const size_t kBlock = 0xd000;
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }
typedef std::vector<uint8_t> Bytes;

static Bytes drawn(size_t n, uint32_t lo, uint32_t span) { Bytes v(n); for (auto &b : v) b = (uint8_t)(lo + rnd() % span); return v; }
static Bytes bam_like(int n_rec) {
  static const uint8_t nib[4] = {1, 2, 4, 8};
  Bytes v;
  for (int i = 0; i < n_rec; ++i) {
    char name[16];
    snprintf(name, sizeof name, "r%09d", i);
    const int32_t head[9] = {3, 1000 + i, (int32_t)(11u | 60u << 8 | 4681u << 16), (int32_t)(1u | 99u << 16), 150, 3, 1300 + i, 450, 0};
    v.insert(v.end(), (const uint8_t *)head, (const uint8_t *)head + 32);
    v.insert(v.end(), name, name + 11);
    for (int k = 0; k < 75; ++k) v.push_back((uint8_t)(nib[rnd() & 3] << 4 | nib[rnd() & 3]));
    for (int k = 0; k < 150; ++k) { int g = 1; while ((rnd() & 3) != 0 && g < 60) ++g; v.push_back((uint8_t)std::min(41, std::max(2, 38 - g))); }      // 38 - geometric(0.25)
    const char tags[] = "XTAUNMC\0SMC%AMC%X0C\1X1C\0XMC\0XOC\0XGC\0MDZ150";
    v.insert(v.end(), tags, tags + sizeof tags);
  }
  return v;
}
static Bytes no_repeat(size_t n) {      // no window of four bytes twice
  std::unordered_set<uint32_t> seen;
  Bytes v;
  while (v.size() < n) {
    const uint8_t c = (uint8_t)rnd();
    if (v.size() >= 3) {
      const uint32_t w = (uint32_t)v[v.size() - 3] << 24 | (uint32_t)v[v.size() - 2] << 16 | (uint32_t)v[v.size() - 1] << 8 | c;
      if (!seen.insert(w).second) continue;
    }
    v.push_back(c);
  }
  return v;
}

static long g_bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_bad; fprintf(stderr, "MISMATCH %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static bool deflate_mode(int entry, const Bytes &in, Bytes *out) {      // entry: -1 the old one, else the mode
  const int64_t cap = (int64_t)(in.size() / kBlock + 2) * 65536;
  out->assign((size_t)cap, 0);
  int64_t n = 0;
  const uint8_t none = 0;
  const uint8_t *src = in.empty() ? &none : in.data();
  const int rc = entry < 0 ? fq_bgzf_deflate_device(0, src, (int64_t)in.size(), out->data(), cap, &n, nullptr) : fq_bgzf_deflate_device_mode(0, entry, src, (int64_t)in.size(), out->data(), cap, &n, nullptr);
  out->resize((size_t)n);
  return rc == 0;
}
// the members' sizes; every member inflated by zlib against its block of the input
static std::vector<size_t> check_members(const char *name, const Bytes &in, const Bytes &z, int *n_dynamic) {
  std::vector<size_t> sizes;
  size_t at = 0, pos = 0;
  *n_dynamic = 0;
  while (at < z.size()) {
    if (at + 28 > z.size() || z[at] != 31 || z[at + 1] != 139 || z[at + 2] != 8 || z[at + 3] != 4 || z[at + 12] != 'B' || z[at + 13] != 'C') { EXPECT(false, "%s: not a BGZF member at %zu", name, at); return sizes; }
    const size_t bs = (size_t)(z[at + 16] | z[at + 17] << 8) + 1;
    if (bs > 65536 || at + bs > z.size()) { EXPECT(false, "%s: BSIZE %zu at %zu", name, bs, at); return sizes; }
    *n_dynamic += (z[at + 18] >> 1 & 3) == 2;
    Bytes back(kBlock + 64);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    inflateInit2(&zs, -15);
    zs.next_in = const_cast<uint8_t *>(z.data() + at + 18); zs.avail_in = (uInt)(bs - 26);
    zs.next_out = back.data(); zs.avail_out = (uInt)back.size();
    const int rc = inflate(&zs, Z_FINISH);
    const size_t got = zs.total_out;
    EXPECT(rc == Z_STREAM_END && zs.avail_in == 0, "%s: zlib says %d for the member at %zu (%u bytes left)", name, rc, at, zs.avail_in);
    inflateEnd(&zs);
    uint32_t crc, isz;
    memcpy(&crc, z.data() + at + bs - 8, 4); memcpy(&isz, z.data() + at + bs - 4, 4);
    const size_t want = std::min(kBlock, in.size() - pos);
    EXPECT(got == want && isz == want && (want == 0 || !memcmp(back.data(), in.data() + pos, want)), "%s: the member at %zu inflates to %zu bytes, ISIZE %u, the block has %zu", name, at, got, isz, want);
    EXPECT(crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), back.data(), (uInt)got), "%s: CRC-32 of the member at %zu", name, at);
    pos += want; at += bs;
    sizes.push_back(bs);
  }
  EXPECT(pos == in.size() && sizes.size() == (in.size() + kBlock - 1) / kBlock, "%s: %zu members for %zu bytes", name, sizes.size(), in.size());
  return sizes;
}
static void check_input(const char *name, const Bytes &in) {
  Bytes old, fixed, dyn;
  EXPECT(deflate_mode(-1, in, &old) && deflate_mode(FQ_DEFLATE_FIXED, in, &fixed) && deflate_mode(FQ_DEFLATE_DYNAMIC, in, &dyn), "%s: an entry failed", name);
  EXPECT(old == fixed, "%s: the fixed mode's bytes are not the old entry's", name);
  int nf = 0, nd = 0;
  const std::vector<size_t> sf = check_members(name, in, fixed, &nf), sd = check_members(name, in, dyn, &nd);
  EXPECT(nf == 0, "%s: a member of the fixed mode says BTYPE = 10", name);
  EXPECT(sf.size() == sd.size(), "%s: member counts", name);
  for (size_t k = 0; k < std::min(sf.size(), sd.size()); ++k) EXPECT(sd[k] <= sf[k], "%s: member %zu is %zu bytes in dynamic mode, %zu in fixed", name, k, sd[k], sf[k]);
  printf("%-22s %8zu bytes: fixed %8zu, dynamic %8zu (%d of %zu members BTYPE = 10)\n", name, in.size(), fixed.size(), dyn.size(), nd, sd.size());
}

// Huffman's cost and depth (a priority queue; ties to the shallower subtree)
static void huffman(const std::vector<uint32_t> &f, uint64_t *cost, int *depth) {
  typedef std::pair<uint64_t, int> Node;      // weight, depth
  std::priority_queue<Node, std::vector<Node>, std::greater<Node>> q;
  for (uint32_t v : f) if (v) q.push(Node(v, 0));
  *cost = 0; *depth = 0;
  while (q.size() > 1) {
    const Node a = q.top(); q.pop();
    const Node b = q.top(); q.pop();
    *cost += a.first + b.first;
    q.push(Node(a.first + b.first, std::max(a.second, b.second) + 1));
  }
  if (!q.empty()) *depth = q.top().second;
}
static void check_lengths(const char *name, const std::vector<uint32_t> &f, int limit) {
  std::vector<uint8_t> len(f.size(), 0xff);
  if (fq_huffman_lengths_device(0, f.data(), (int)f.size(), limit, len.data())) { EXPECT(false, "%s: the entry failed", name); return; }
  uint64_t kraft = 0, cost = 0, flat = 0;
  int used = 0, coded = 0;
  for (size_t s = 0; s < f.size(); ++s) {
    EXPECT(len[s] <= limit && (!f[s] || len[s] >= 1), "%s: symbol %zu of frequency %u has length %d", name, s, f[s], len[s]);
    if (len[s] && len[s] <= limit) { kraft += 1ull << (limit - len[s]); ++coded; }
    used += f[s] != 0; cost += (uint64_t)f[s] * len[s]; flat += f[s];
  }
  EXPECT(kraft == 1ull << limit, "%s: the Kraft sum is %llu / %llu", name, (unsigned long long)kraft, 1ull << limit);
  EXPECT(coded == std::max(used, 2), "%s: %d codes for %d used symbols", name, coded, used);
  if (used < 2) return;
  uint64_t hc; int hd;
  huffman(f, &hc, &hd);
  int flat_bits = 1;
  while ((1 << flat_bits) < used) ++flat_bits;
  if (hd <= limit) EXPECT(cost == hc, "%s: %llu bits, Huffman's code costs %llu", name, (unsigned long long)cost, (unsigned long long)hc);
  else { EXPECT(cost >= hc && cost <= flat * flat_bits, "%s: %llu bits beyond the limit (Huffman %llu, flat %llu)", name, (unsigned long long)cost, (unsigned long long)hc, (unsigned long long)(flat * flat_bits));
         printf("%-22s limit %2d: Huffman %llu bits at depth %d, the repair %llu\n", name, limit, (unsigned long long)hc, hd, (unsigned long long)cost); }
}

int main() {
  // ---- test 1's inputs
  Bytes runs;
  for (int k = 0; k < 70000; ++k) { runs.push_back('a'); runs.push_back('b'); }
  runs.insert(runs.end(), 300, 'c');
  Bytes far = drawn(40000, 0, 256), far3;
  for (int k = 0; k < 3; ++k) far3.insert(far3.end(), far.begin(), far.end());
  Bytes text;
  for (int k = 0; k < 5000; ++k) { const char *l = "@r000000001\nACGTACGTTTGACCA\n+\nFFFFFFFFFFFFFF:\n"; text.insert(text.end(), l, l + strlen(l)); }
  Bytes two = drawn(kBlock, 0, 2);
  for (auto &b : two) b = b ? 200 : 65;
  const std::pair<const char *, Bytes> inputs[] = {
    {"empty", Bytes()}, {"one_byte", Bytes(1, 'A')}, {"AAA", Bytes(3, 'A')}, {"zeros", Bytes(200000, 0)}, {"random", drawn(150000, 0, 256)}, {"nine_bit_literals", drawn(3 * kBlock, 144, 112)},
    {"fastq_text", text}, {"bam_like_skewed", bam_like(3000)}, {"exact_block", drawn(kBlock, 0, 4)}, {"block_plus_one", drawn(kBlock + 1, 0, 4)}, {"block_minus_one", drawn(kBlock - 1, 0, 7)},
    {"long_runs", runs}, {"far_repeats", far3}, {"one_byte_repeated", Bytes(kBlock, 'Q')}, {"two_values", two}, {"no_four_byte_repeat", no_repeat(kBlock)},
  };
  for (const auto &c : inputs) check_input(c.first, c.second);
  // ---- test 5's frequency vectors
  const int shapes[3][2] = {{286, 15}, {30, 15}, {19, 7}};
  for (const auto &sh : shapes) {
    const int n = sh[0], limit = sh[1];
    std::vector<uint32_t> f((size_t)n, 0);
    check_lengths("all_zero", f, limit);
    f[(size_t)n / 3] = 9; check_lengths("one_used", f, limit);
    f.assign((size_t)n, 0); f[0] = 4; check_lengths("only_symbol_0", f, limit);
    f.assign((size_t)n, 0); f[1] = 4; check_lengths("only_symbol_1", f, limit);
    f.assign((size_t)n, 0); f[2] = 1; f[(size_t)n - 1] = 1000; check_lengths("two_used", f, limit);
    f.assign((size_t)n, 3); check_lengths("all_equal", f, limit);
  }
  std::vector<uint32_t> p2(30, 0), fib(24, 1);
  for (int k = 0; k < 20; ++k) p2[(size_t)k] = 1u << k;
  check_lengths("powers_of_two_20", p2, 15);
  for (size_t k = 2; k < fib.size(); ++k) fib[k] = fib[k - 1] + fib[k - 2];
  check_lengths("fibonacci_24", fib, 15);
  fib.resize(19);
  check_lengths("fibonacci_19", fib, 7);
  for (int k = 0; k < 20; ++k) {
    const int n = shapes[k % 3][0], limit = shapes[k % 3][1], bits = 1 + (int)(rnd() % 16), keep = (int)(rnd() % 3);
    std::vector<uint32_t> f((size_t)n);
    for (auto &v : f) v = (rnd() % 10 < (keep == 0 ? 1u : keep == 1 ? 4u : 9u)) ? rnd() & ((1u << bits) - 1) : 0;
    check_lengths(("random_" + std::to_string(k)).c_str(), f, limit);
  }
  if (g_bad) { fprintf(stderr, "%ld mismatches\n", g_bad); return 1; }
  printf("ok\n");
  return 0;
}
