// Measures, on the GPU it runs on, (1) device-to-device stream copy bandwidth and (2) the rate of isolated random one-byte
// probes into a 3 GiB table with 18 independent probes in flight per thread: the access pattern of the k-mer filter.
// (2) is the practical ceiling for the filter kernel: every probe moves one 64-byte line.
// (3) the same probes at the filter's shape (8 Mi reads, 16 probes each, six 512 MiB bitmaps), direct against binned by 2 MiB
// region: count + scan + bin + probe + mask read-back as separate launches, each timed, and the hit masks of the two forms compared.
//   hipcc --offload-arch=gfx950 -O3 -o hbm_probe_bench tools/hbm_probe_bench.hip && ./hbm_probe_bench
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void k_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}
__device__ inline uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return x; }
template <int P>
__global__ void k_probe(const uint8_t *__restrict__ tab, uint64_t mask, uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint8_t v[P];
#pragma unroll
  for (int p = 0; p < P; ++p) v[p] = tab[mix((uint64_t)t * P + p + 1) & mask];
  uint32_t s = 0;
#pragma unroll
  for (int p = 0; p < P; ++p) s += v[p];
  out[t] = s;
}

// ---- (3) the filter's shape -----------------------------------------------------------------------------------------------------
// Read r issues NQ probes; probe q goes to table q % 6 with the 32-bit key key_of(r, q): bit key & 7 of byte key >> 3 of that table.
// A bucket is one 2 MiB region (2^24 bits) of one table: 6 x 256 buckets.  Buckets are laid out XCD-major, bucket b at position
// (b % 8) * 192 + b / 8, so that the probe launch's workgroups with blockIdx % 8 == x walk the buckets of one list in order.
constexpr int NQ = 16, NB = 6 * 256, NXCD = 8, PER_XCD = NB / NXCD;
constexpr uint32_t kTabBytes = 1u << 29;
__device__ inline uint32_t key_of(uint32_t r, int q) { return (uint32_t)mix((uint64_t)r * NQ + q + 1); }
__device__ inline int pos_of(int t, uint32_t key) { const int b = t * 256 + (int)(key >> 24); return (b % NXCD) * PER_XCD + b / NXCD; }

__global__ void k_fill_sparse(uint4 *__restrict__ tab, size_t n) {   // about 0.4 % of the bits set
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t a = ~0ull, b = ~0ull;
    for (int j = 0; j < 8; ++j) { a &= mix(i * 16 + j + 1); b &= mix(i * 16 + 8 + j + 1); }
    tab[i] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  }
}
__global__ void __launch_bounds__(256) k_direct16(const uint8_t *__restrict__ tab, uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint32_t key[NQ]; uint8_t v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) { key[q] = key_of(r, q); v[q] = tab[(size_t)(q % 6) * kTabBytes + (key[q] >> 3)]; }
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) m |= (uint32_t)((v[q] >> (key[q] & 7u)) & 1u) << q;
  out[r] = m;
}
// count: entries per bucket.  Persistent workgroups, one flush of the LDS histogram each.
__global__ void __launch_bounds__(1024) k_bin_count(uint32_t *__restrict__ count, uint32_t n) {
  __shared__ uint32_t h[NB];
  for (int i = threadIdx.x; i < NB; i += blockDim.x) h[i] = 0;
  __syncthreads();
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
#pragma unroll
    for (int q = 0; q < NQ; ++q) atomicAdd(&h[pos_of(q % 6, key_of(r, q))], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < NB; i += blockDim.x) if (h[i]) atomicAdd(&count[i], h[i]);
}
// scan: base[p] = first entry of position p, cursor[p] = base[p], cp[p] = chunks before p (chunks of `chunk` entries); one workgroup
__global__ void __launch_bounds__(256) k_bin_scan(const uint32_t *__restrict__ count, uint32_t *__restrict__ base, uint32_t *__restrict__ cursor,
                                                  uint32_t *__restrict__ cp, uint32_t chunk) {
  __shared__ uint32_t se[256], sc[256];
  const int t = threadIdx.x;
  uint32_t c[6], e = 0, k = 0;
  for (int j = 0; j < 6; ++j) { c[j] = count[6 * t + j]; e += c[j]; k += (c[j] + chunk - 1) / chunk; }
  se[t] = e; sc[t] = k;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint32_t ae = t >= d ? se[t - d] : 0, ac = t >= d ? sc[t - d] : 0;
    __syncthreads();
    se[t] += ae; sc[t] += ac;
    __syncthreads();
  }
  e = se[t] - e; k = sc[t] - k;
  for (int j = 0; j < 6; ++j) { base[6 * t + j] = e; cursor[6 * t + j] = e; cp[6 * t + j] = k; e += c[j]; k += (c[j] + chunk - 1) / chunk; }
  if (t == 255) { base[NB] = e; cp[NB] = k; }
}
// bin: a tile of RPT * 1024 reads per step, one table at a time: counting sort by the key's top byte in LDS, one claim per bucket
// with entries, then the sorted tile leaves as runs of consecutive 8-byte entries.  Entry: x = key, y = read << 5 | probe.
template <int RPT>
__global__ void __launch_bounds__(1024) k_bin(uint2 *__restrict__ ent, uint32_t *__restrict__ cursor, uint32_t n) {
  constexpr int TILE = RPT * 1024, MAXE = TILE * 3;
  __shared__ uint2 sorted[MAXE];
  __shared__ uint32_t h[256], start[256], delta[256];
  const int tid = threadIdx.x;
  const uint32_t n_tiles = (n + TILE - 1) / TILE;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    for (int t = 0; t < 6; ++t) {
      const int nq = t < NQ % 6 ? NQ / 6 + 1 : NQ / 6;   // probes q = t, t + 6, ... < NQ
      if (tid < 256) h[tid] = 0;
      __syncthreads();
      uint32_t key[RPT][3], rank[RPT][3];
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const uint32_t r = tile * TILE + i * 1024 + tid;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < nq && r < n) { key[i][j] = key_of(r, t + 6 * j); rank[i][j] = atomicAdd(&h[key[i][j] >> 24], 1u); }
      }
      __syncthreads();
      if (tid < 256) start[tid] = h[tid];
      __syncthreads();
      for (int d = 1; d < 256; d <<= 1) {
        const uint32_t a = (tid < 256 && tid >= d) ? start[tid - d] : 0;
        __syncthreads();
        if (tid < 256) start[tid] += a;
        __syncthreads();
      }
      if (tid < 256) {
        const uint32_t c = h[tid], s = start[tid] - c;
        start[tid] = s;
        if (c) delta[tid] = atomicAdd(&cursor[pos_of(t, (uint32_t)tid << 24)], c) - s;
      }
      __syncthreads();
      const uint32_t n_ent = start[255] + h[255];
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const uint32_t r = tile * TILE + i * 1024 + tid;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < nq && r < n) sorted[start[key[i][j] >> 24] + rank[i][j]] = make_uint2(key[i][j], r << 5 | (uint32_t)(t + 6 * j));
      }
      __syncthreads();
      for (uint32_t i = tid; i < n_ent; i += 1024) { const uint2 e = sorted[i]; ent[delta[e.x >> 24] + i] = e; }
      __syncthreads();
    }
  }
}
// probe: persistent workgroups; those with blockIdx % 8 == x take the chunks of list x in order, so the chunks in flight on one XCD
// belong to one or two neighbouring buckets and their 2 MiB regions stay in that XCD's L2.
template <int E>
__global__ void __launch_bounds__(512) k_bin_probe(const uint8_t *__restrict__ tab, const uint2 *__restrict__ ent, const uint32_t *__restrict__ base,
                                                   const uint32_t *__restrict__ cp, uint32_t *__restrict__ mask) {
  constexpr uint32_t CH = 512 * E;
  const int x = blockIdx.x % NXCD;
  const uint32_t per = gridDim.x / NXCD, c0 = cp[x * PER_XCD], c1 = cp[(x + 1) * PER_XCD];
  for (uint32_t k = c0 + blockIdx.x / NXCD; k < c1; k += per) {
    int lo = x * PER_XCD, hi = (x + 1) * PER_XCD;      // the last position with cp[p] <= k
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (cp[mid] <= k) lo = mid; else hi = mid; }
    const int b = (lo % PER_XCD) * NXCD + x;
    const uint8_t *reg = tab + (size_t)(b >> 8) * kTabBytes + ((size_t)(b & 255) << 21);
    const uint32_t first = base[lo] + (k - cp[lo]) * CH, end = base[lo + 1];
    uint2 e[E]; uint8_t v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) { const uint32_t at = first + i * 512 + threadIdx.x; e[i] = at < end ? ent[at] : make_uint2(0, ~0u); }
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = e[i].y != ~0u ? reg[(e[i].x & 0xffffffu) >> 3] : 0;
#pragma unroll
    for (int i = 0; i < E; ++i) if ((v[i] >> (e[i].x & 7u)) & 1u) atomicOr(&mask[e[i].y >> 5], 1u << (e[i].y & 31u));
  }
}
__global__ void __launch_bounds__(256) k_bin_verdict(uint32_t *__restrict__ mask, uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  out[r] = mask[r]; mask[r] = 0;
}
__global__ void k_diff(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t n, uint32_t *__restrict__ res) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (a[r] != b[r]) atomicAdd(&res[0], 1u);
  if (a[r]) atomicAdd(&res[1], (uint32_t)__popc(a[r]));
}

template <int RPT, int E>
static void run_binned(const uint8_t *tab, uint32_t n, const uint32_t *ref, int wg_per_xcd) {
  uint2 *ent; uint32_t *count, *base, *cursor, *cp, *mask, *out, *res;
  CK(hipMalloc(&ent, (size_t)n * NQ * 8)); CK(hipMalloc(&count, NB * 4)); CK(hipMalloc(&base, (NB + 1) * 4)); CK(hipMalloc(&cursor, NB * 4));
  CK(hipMalloc(&cp, (NB + 1) * 4)); CK(hipMalloc(&mask, (size_t)n * 4)); CK(hipMalloc(&out, (size_t)n * 4)); CK(hipMalloc(&res, 8));
  CK(hipMemset(mask, 0, (size_t)n * 4));
  hipEvent_t ev[6]; for (auto &e : ev) CK(hipEventCreate(&e));
  for (int it = 0; it < 4; ++it) {
    CK(hipMemsetAsync(out, 0xff, (size_t)n * 4));
    CK(hipEventRecord(ev[0]));
    CK(hipMemsetAsync(count, 0, NB * 4));
    hipLaunchKernelGGL(k_bin_count, dim3(512), dim3(1024), 0, 0, count, n);
    CK(hipEventRecord(ev[1]));
    hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(256), 0, 0, count, base, cursor, cp, (uint32_t)(512 * E));
    CK(hipEventRecord(ev[2]));
    hipLaunchKernelGGL((k_bin<RPT>), dim3(512), dim3(1024), 0, 0, ent, cursor, n);
    CK(hipEventRecord(ev[3]));
    hipLaunchKernelGGL((k_bin_probe<E>), dim3(NXCD * wg_per_xcd), dim3(512), 0, 0, tab, ent, base, cp, mask);
    CK(hipEventRecord(ev[4]));
    hipLaunchKernelGGL(k_bin_verdict, dim3((n + 255) / 256), dim3(256), 0, 0, mask, out, n);
    CK(hipEventRecord(ev[5]));
    CK(hipEventSynchronize(ev[5]));
    float ms[5], tot;
    for (int i = 0; i < 5; ++i) CK(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    CK(hipEventElapsedTime(&tot, ev[0], ev[5]));
    uint32_t h[2];
    CK(hipMemset(res, 0, 8));
    hipLaunchKernelGGL(k_diff, dim3((n + 255) / 256), dim3(256), 0, 0, ref, out, n, res);
    CK(hipMemcpy(h, res, 8, hipMemcpyDeviceToHost));
    printf("binned, tile %d reads, %d entries per thread, %d workgroups per XCD: count %.3f scan %.3f bin %.3f probe %.3f verdict %.3f  total %.3f ms"
           "  %.2f G probes/s  (%u of %u masks differ from the direct form, %u hits)\n",
           RPT * 1024, E, wg_per_xcd, ms[0], ms[1], ms[2], ms[3], ms[4], tot, (double)NQ * n / (tot * 1e-3) / 1e9, h[0], n, h[1]);
  }
  for (auto &e : ev) CK(hipEventDestroy(e));
  CK(hipFree(ent)); CK(hipFree(count)); CK(hipFree(base)); CK(hipFree(cursor)); CK(hipFree(cp)); CK(hipFree(mask)); CK(hipFree(out)); CK(hipFree(res));
}

int main() {
  const size_t bytes = (size_t)3 << 30;
  uint8_t *a, *b; uint32_t *out;
  CK(hipMalloc(&a, bytes)); CK(hipMalloc(&b, bytes)); CK(hipMemset(a, 1, bytes));
  const uint32_t n = 8u << 20;
  CK(hipMalloc(&out, (size_t)n * 4));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float ms;
  for (int it = 0; it < 3; ++it) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_copy, dim3(256 * 32), dim3(256), 0, 0, (const uint4 *)a, (uint4 *)b, bytes / 16);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
    printf("stream copy 3 GiB: %.3f ms  read+write %.2f TB/s\n", ms, 2.0 * bytes / (ms * 1e-3) / 1e12);
  }
  const uint64_t masks[2] = {((uint64_t)2 << 30) - 1, ((uint64_t)256 << 20) - 1};   // 2 GiB span (power of two inside the table), 256 MiB span
  for (int m = 0; m < 2; ++m)
    for (int it = 0; it < 3; ++it) {
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL(k_probe<18>, dim3((n + 255) / 256), dim3(256), 0, 0, a, masks[m], out, n);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
      printf("random probes over %4llu MiB, 18 per thread, %u threads: %.3f ms  %.2f G probes/s  = %.2f TB/s of 64-byte lines\n",
             (unsigned long long)((masks[m] + 1) >> 20), n, ms, 18.0 * n / (ms * 1e-3) / 1e9, 64.0 * 18.0 * n / (ms * 1e-3) / 1e12);
    }
  // (3) the filter's shape: b is free now, the tables go into a
  CK(hipFree(b));
  hipLaunchKernelGGL(k_fill_sparse, dim3(256 * 32), dim3(256), 0, 0, (uint4 *)a, bytes / 16);
  CK(hipDeviceSynchronize());
  for (int it = 0; it < 4; ++it) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_direct16, dim3((n + 255) / 256), dim3(256), 0, 0, a, out, n);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
    printf("direct, six 512 MiB tables, %d per thread, %u threads: %.3f ms  %.2f G probes/s\n", NQ, n, ms, (double)NQ * n / (ms * 1e-3) / 1e9);
  }
  // (entries per thread, workgroups per XCD): 32 workgroups of 512 threads per XCD are one per CU
  run_binned<2, 2>(a, n, out, 32);
  run_binned<2, 4>(a, n, out, 32);
  run_binned<2, 8>(a, n, out, 32);
  run_binned<2, 4>(a, n, out, 16);
  run_binned<2, 4>(a, n, out, 24);
  run_binned<2, 2>(a, n, out, 64);
  run_binned<1, 1>(a, n, out, 64);
  return 0;
}
