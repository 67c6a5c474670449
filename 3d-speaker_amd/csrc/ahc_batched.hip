// Batched average-linkage AHC: the loop of ahc.hip (same algorithm, state, tie rule and update,
// DESIGN §7 'Device AHC') with one workgroup per problem and the whole merge loop inside one
// launch.  select, merge and repair are phases of that workgroup separated by workgroup barriers
// where ahc.hip has launch boundaries; the per-row caches, sizes, the active mask, the member map
// and the stale list live in LDS (28 N bytes + 4.4 KB), the fp64 working matrix in the caller's
// workspace, written and re-read by this workgroup only.  One difference in how, not what: row i's
// new cache is reduced from the values merge has in registers (a workgroup reduction, which
// ahc.hip's many merge workgroups cannot do) and not rescanned from memory; it is the same entry.
//
// No workgroup waits on another one (no grid barrier, no flag spin, no cooperative launch): a
// problem's workgroup exits when its loop ends.  The loop runs at most N - 1 times and every inner
// loop is bounded by N whatever the data holds (NaN similarities end the loop at the first select:
// no value is >= the threshold).
#include "ahc.h"
#include "ahc_dev.h"

#include <algorithm>

namespace spk {

namespace {

// A = double(S[min(r, c)][max(r, c)]) for every problem of the chunk (blockIdx.z): the upper
// triangle mirrored, as ahc.hip's convert
__global__ void __launch_bounds__(256) ahc_batched_convert_kernel(AhcBatchArgs a) {
  __shared__ float t[32][33];
  const AhcBatchProb& pb = a.p[blockIdx.z];
  const float* __restrict__ S = pb.S;
  double* __restrict__ A = pb.A;
  const long long N = pb.N, lds = pb.lds;
  const long long bi = blockIdx.y * 32LL, bj = blockIdx.x * 32LL;
  if (bi > bj || bj >= N) return;   // the grid is sized by the chunk's largest problem
  const int tx = threadIdx.x, ty = threadIdx.y;   // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const long long i = bi + r, j = bj + tx;
    t[r][tx] = (i < N && j < N) ? S[i * lds + j] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const long long i = bi + r, j = bj + tx;
    if (i < N && j < N) A[i * N + j] = (double)(i <= j ? t[r][tx] : t[tx][r]);
  }
  if (bi != bj)
    for (int r = ty; r < 32; r += 8) {
      const long long i = bj + r, j = bi + tx;   // the mirrored tile: A[i][j] = S[j][i]
      if (i < N && j < N) A[i * N + j] = (double)t[tx][r];
    }
}

constexpr int BT = 1024;       // threads of a problem's workgroup
constexpr int BW = BT / 64;    // its waves: repair rescans one stale row per wave

// LDS control words
enum { B_RUN = 0, B_I, B_J, B_SI, B_SJ, B_NSTALE, B_NACTIVE, B_WORDS = 8 };

struct Lds {
  Cand* slots;   // [BW]
  double* val;   // [N] row r's best A[r][c] over the active c > r ...
  int* col;      // [N] ... and its (smallest) column, -1: none
  int* size;     // [N]
  int* active;   // [N]
  int* member;   // [N] cluster of input row r
  int* stale;    // [N] rows repair rescans; the epilogue's rank
  int* scan;     // [BT]
  int* ctrl;     // [B_WORDS]
};

__host__ __device__ constexpr size_t lds_bytes(int N) {
  return BW * sizeof(Cand) + (size_t)N * (sizeof(double) + 5 * sizeof(int)) + (BT + B_WORDS) * sizeof(int);
}

__device__ __forceinline__ Lds carve(char* base, int N) {
  Lds l;
  l.slots = reinterpret_cast<Cand*>(base);
  l.val = reinterpret_cast<double*>(l.slots + BW);
  l.col = reinterpret_cast<int*>(l.val + N);
  l.size = l.col + N;
  l.active = l.size + N;
  l.member = l.active + N;
  l.stale = l.member + N;
  l.scan = l.stale + N;
  l.ctrl = l.scan + BT;
  return l;
}

__device__ __forceinline__ void mark_stale(const Lds& l, int N, int k) {
  const int p = atomicAdd(l.ctrl + B_NSTALE, 1);   // an LDS atomic
  if (p < N) l.stale[p] = k;   // at most one entry per row and step: p < N always
}

// this wave rescans row r over the active columns above it; lane 0 writes the cache
__device__ __forceinline__ void rescan_row(const Lds& l, const double* A, int N, int r) {
  const double* row = A + (size_t)r * N;
  const int lane = threadIdx.x & 63;
  Cand best{0.0, r, -1};
  constexpr int U = 4;   // independent loads in flight per lane: the scan is latency-bound
  for (int c0 = r + 1 + lane; c0 < N; c0 += 64 * U) {   // ascending c: a tie keeps the smaller column
    double v[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + 64 * u;
      on[u] = c < N && l.active[c];
      v[u] = c < N ? row[c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (on[u] && (best.c < 0 || v[u] > best.v)) {
        best.v = v[u];
        best.c = c0 + 64 * u;
      }
  }
  best = wave_best(best);
  if (lane == 0) {
    l.val[r] = best.v;
    l.col[r] = best.c;
  }
}

__global__ void __launch_bounds__(BT) ahc_batched_kernel(AhcBatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ahc_lds[];
  const AhcBatchProb& pb = a.p[blockIdx.x];
  const int N = pb.N;
  const double thr = (double)pb.thr;
  double* A = pb.A;
  const Lds l = carve(ahc_lds, N);
  const int tid = threadIdx.x, wave = tid >> 6;

  for (int r = tid; r < N; r += BT) {
    l.size[r] = 1;
    l.active[r] = 1;
    l.member[r] = r;
  }
  if (tid == 0) {
    l.ctrl[B_RUN] = 1;
    l.ctrl[B_NSTALE] = 0;
    l.ctrl[B_NACTIVE] = N;
  }
  __syncthreads();
  for (int r = wave; r < N; r += BW) rescan_row(l, A, N, r);   // every row's cache
  __syncthreads();

  for (int step = 0; step + 1 < N; ++step) {
    // ---- select: the best cached pair (i, j)
    Cand best{0.0, 0, -1};
    for (int r = tid; r < N; r += BT) {
      if (!l.active[r]) continue;
      const Cand c{l.val[r], r, l.col[r]};
      if (beats(best, c)) best = c;
    }
    best = block_best<BT>(best, l.slots);
    if (tid == 0) {
      const int nact = l.ctrl[B_NACTIVE];
      if (nact <= 1 || best.c < 0 || !(best.v >= thr)) {
        l.ctrl[B_RUN] = 0;
      } else {
        const int i = best.r, j = best.c, si = l.size[i], sj = l.size[j];
        l.ctrl[B_I] = i;
        l.ctrl[B_J] = j;
        l.ctrl[B_SI] = si;
        l.ctrl[B_SJ] = sj;
        l.ctrl[B_NSTALE] = 0;
        l.ctrl[B_NACTIVE] = nact - 1;
        l.size[i] = si + sj;
        l.active[j] = 0;
      }
    }
    __syncthreads();
    if (!l.ctrl[B_RUN]) break;   // the same word for every thread: the workgroup leaves together

    // ---- merge: one thread per k, as ahc.hip's merge kernel
    const int i = l.ctrl[B_I], j = l.ctrl[B_J], si = l.ctrl[B_SI], sj = l.ctrl[B_SJ];
    const size_t n = (size_t)N;
    Cand rowi{0.0, i, -1};   // row i changed everywhere: its new cache is the best of what merge writes
    for (int k = tid; k < N; k += BT) {
      if (l.member[k] == j) l.member[k] = i;
      if (k == i || k == j || !l.active[k]) continue;
      const double v = lance_williams(A[i * n + k], A[j * n + k], si, sj);
      A[i * n + k] = v;
      A[k * n + i] = v;
      if (k > i && (rowi.c < 0 || v > rowi.v)) {   // ascending k: a tie keeps the smaller column
        rowi.v = v;
        rowi.c = k;
      }
      if (k < i) {   // columns i and j are both in row k's range
        const int cc = l.col[k];
        const double cv = l.val[k];
        if (cc == j) {
          mark_stale(l, N, k);
        } else if (cc == i) {
          if (v >= cv) l.val[k] = v;   // still the best: every other entry is <= cv
          else mark_stale(l, N, k);
        } else if (cc < 0 || v > cv || (v == cv && i < cc)) {
          l.val[k] = v;
          l.col[k] = i;
        }
      } else if (k < j) {   // only column j is
        if (l.col[k] == j) mark_stale(l, N, k);
      }
    }
    rowi = block_best<BT>(rowi, l.slots);   // what a rescan of row i would find, without re-reading it
    if (tid == 0) {
      l.val[i] = rowi.v;
      l.col[i] = rowi.c;
    }
    // The matrix entries merge stored are read below by other waves of this workgroup.  A
    // workgroup barrier is enough for that: __syncthreads() is a workgroup-scope release (each
    // wave waits for its own stores, vmcnt(0)), the barrier, and a workgroup-scope acquire, and
    // the waves of a workgroup run on one CU, whose L1 is the only cache that is not shared
    // with the writer.  Nothing here is read by another workgroup, so no agent-scope fence.
    __syncthreads();

    // ---- repair: one wave per stale row
    const int ns = min(l.ctrl[B_NSTALE], N);
    for (int idx = wave; idx < ns; idx += BW) rescan_row(l, A, N, l.stale[idx]);
    __syncthreads();
  }

  // ---- labels[r] = number of clusters whose index is below r's cluster (ahc.hip's labels kernel)
  const int chunk = (N + BT - 1) / BT;
  const int lo = min(tid * chunk, N), hi = min(lo + chunk, N);
  int cnt = 0;
  for (int q = lo; q < hi; ++q) cnt += l.active[q];
  l.scan[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < BT; off <<= 1) {
    const int add = tid >= off ? l.scan[tid - off] : 0;
    __syncthreads();
    l.scan[tid] += add;
    __syncthreads();
  }
  int run = l.scan[tid] - cnt;
  int* rank = l.stale;
  for (int q = lo; q < hi; ++q) {
    rank[q] = run;
    run += l.active[q];
  }
  __syncthreads();
  for (int r = tid; r < N; r += BT) pb.labels[r] = rank[l.member[r]];
  if (tid == 0) a.n_clusters[blockIdx.x] = l.scan[BT - 1];
}

}  // namespace

hipError_t launch_ahc_batched(const AhcBatchArgs& a, hipStream_t s) {
  static_assert(sizeof(AhcBatchArgs) <= 4096, "the descriptors travel as kernel arguments");
  static_assert(lds_bytes(SPK_AHC_BATCH_MAX_N) <= 160 * 1024, "the state of the largest problem fits the CU's LDS");
  if (a.n < 1 || a.n > kAhcBatchChunk) return hipErrorInvalidValue;
  int maxn = 1;
  for (int q = 0; q < a.n; ++q) maxn = std::max(maxn, a.p[q].N);
  const size_t lds = lds_bytes(maxn);   // every workgroup carves by its own N <= maxn
  if (lds > 64 * 1024)   // above the default limit of a launch's dynamic LDS
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ahc_batched_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return e;
  const unsigned nb = (unsigned)((maxn + 31) / 32);
  hipLaunchKernelGGL(ahc_batched_convert_kernel, dim3(nb, nb, (unsigned)a.n), dim3(32, 8), 0, s, a);
  hipLaunchKernelGGL(ahc_batched_kernel, dim3((unsigned)a.n), dim3(BT), lds, s, a);
  return hipGetLastError();
}

}  // namespace spk
