// Average-linkage agglomerative clustering of a cosine affinity on the GPU (reference
// speakerlab/process/cluster.py AHCluster :139-156: fastcluster linkage(method='average') on -S,
// fcluster(criterion='distance') at -fix_cos_thr).
//
// Average linkage is monotone, so the flat clusters of that cut are what the greedy loop leaves:
// merge the two clusters with the largest average similarity until that value is below the
// threshold.  Ties: the largest value, then the smallest row, then the smallest column (row <
// column); the merged cluster keeps the smaller index, so a cluster's index is its smallest
// member and the first-occurrence label of a row is the number of clusters below its own.
//
// The working matrix is fp64 (scipy updates in double too: merge heights agree to rounding) and
// symmetric; row r caches its best entry over the active columns above r.  One merge is three
// launches on the caller's stream, each gated on the run word (SPK_GATE):
//   select  one workgroup: the best cached pair (i, j); below the threshold -> run = 0, else
//           retire j, size[i] += size[j];
//   merge   one thread per k: A[i][k] = A[k][i] = (si A[i][k] + sj A[j][k]) / (si + sj) (written
//           without contraction, the rounding of the numpy restatement in tests/test_gpu_ahc.py);
//           row k < i raises its cache if the new A[k][i] beats it; rows whose cached column was
//           j (or was i and got smaller) and row i itself go on the stale list;
//   repair  a workgroup per stale row rescans it over the active columns above it.
// No kernel waits on another workgroup and every loop is bounded by N.
#include "ahc.h"
#include "ahc_dev.h"

#include <algorithm>

namespace spk {

namespace {

// A = double(S[min(r, c)][max(r, c)]): the upper triangle, which is what squareform() hands the
// host linkage, mirrored so that the matrix is symmetric to the bit
__global__ void __launch_bounds__(256) ahc_convert_kernel(const float* __restrict__ S, long long N, long long lds,
                                                          double* __restrict__ A) {
  __shared__ float t[32][33];
  const long long bi = blockIdx.y * 32LL, bj = blockIdx.x * 32LL;
  if (bi > bj) return;
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

__global__ void __launch_bounds__(256) ahc_state_kernel(AhcState st, int N) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < N) {
    st.size[r] = 1;
    st.active[r] = 1;
    st.member[r] = r;
    st.stale[r] = r;   // the first repair fills every cache
    st.val[r] = 0.0;
    st.col[r] = -1;
  }
  if (r == 0) {
    for (int q = 0; q < AHC_CTRL_WORDS; ++q) st.ctrl[q] = 0;
    st.ctrl[AHC_RUN] = 1;
    st.ctrl[AHC_NSTALE] = N;
    st.ctrl[AHC_NACTIVE] = N;
  }
}

constexpr int ST = 1024;   // select: one workgroup
__global__ void __launch_bounds__(ST) ahc_select_kernel(AhcState st, int N, double thr) {
  SPK_GATE(st.ctrl + AHC_RUN);
  __shared__ Cand slots[ST / 64];
  Cand best{0.0, 0, -1};
  for (int r = threadIdx.x; r < N; r += ST) {
    if (!st.active[r]) continue;
    const Cand c{st.val[r], r, st.col[r]};
    if (beats(best, c)) best = c;
  }
  best = block_best<ST>(best, slots);
  if (threadIdx.x != 0) return;
  const int nact = st.ctrl[AHC_NACTIVE];
  if (nact <= 1 || best.c < 0 || !(best.v >= thr)) {
    st.ctrl[AHC_RUN] = 0;
    return;
  }
  const int i = best.r, j = best.c, si = st.size[i], sj = st.size[j];
  st.ctrl[AHC_I] = i;
  st.ctrl[AHC_J] = j;
  st.ctrl[AHC_SI] = si;
  st.ctrl[AHC_SJ] = sj;
  st.ctrl[AHC_NSTALE] = 0;
  st.ctrl[AHC_NACTIVE] = nact - 1;
  st.ctrl[AHC_STEPS] += 1;
  st.size[i] = si + sj;
  st.active[j] = 0;
}

__device__ __forceinline__ void mark_stale(const AhcState& st, int N, int k) {
  const int p = atomicAdd(st.ctrl + AHC_NSTALE, 1);
  if (p < N) st.stale[p] = k;   // at most one entry per row and step: p < N always
}

__global__ void __launch_bounds__(256) ahc_merge_kernel(AhcState st, int N) {
  SPK_GATE(st.ctrl + AHC_RUN);
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  const int i = st.ctrl[AHC_I], j = st.ctrl[AHC_J], si = st.ctrl[AHC_SI], sj = st.ctrl[AHC_SJ];
  if (st.member[k] == j) st.member[k] = i;
  if (k == i) {
    mark_stale(st, N, i);   // row i changed everywhere: repair rescans it
    return;
  }
  if (k == j || !st.active[k]) return;
  const size_t n = (size_t)N;
  const double v = lance_williams(st.A[i * n + k], st.A[j * n + k], si, sj);
  st.A[i * n + k] = v;
  st.A[k * n + i] = v;
  if (k < i) {   // columns i and j are both in row k's range
    const int cc = st.col[k];
    const double cv = st.val[k];
    if (cc == j) {
      mark_stale(st, N, k);
    } else if (cc == i) {
      if (v >= cv) st.val[k] = v;   // still the best: every other entry is <= cv
      else mark_stale(st, N, k);
    } else if (cc < 0 || v > cv || (v == cv && i < cc)) {
      st.val[k] = v;
      st.col[k] = i;
    }
  } else if (k < j) {   // only column j is
    if (st.col[k] == j) mark_stale(st, N, k);
  }
}

constexpr int RT = 512;
__global__ void __launch_bounds__(RT) ahc_repair_kernel(AhcState st, int N) {
  SPK_GATE(st.ctrl + AHC_RUN);
  __shared__ Cand slots[RT / 64];
  const int ns = min(st.ctrl[AHC_NSTALE], N);
  for (int idx = blockIdx.x; idx < ns; idx += gridDim.x) {
    const int r = st.stale[idx];
    const double* row = st.A + (size_t)r * N;
    Cand best{0.0, r, -1};
    for (int c = r + 1 + threadIdx.x; c < N; c += RT) {   // ascending c: a tie keeps the smaller column
      if (!st.active[c]) continue;
      const double v = row[c];
      if (best.c < 0 || v > best.v) {
        best.v = v;
        best.c = c;
      }
    }
    best = block_best<RT>(best, slots);
    if (threadIdx.x == 0) {
      st.val[r] = best.v;
      st.col[r] = best.c;
    }
    __syncthreads();   // slots are reused by the next row
  }
}

// labels[r] = number of clusters whose index is below r's cluster (first occurrence: a
// cluster's index is its smallest member)
constexpr int LT = 1024;
__global__ void __launch_bounds__(LT) ahc_labels_kernel(AhcState st, int N, int32_t* __restrict__ labels,
                                                        int32_t* __restrict__ n_clusters) {
  __shared__ int scan[LT];
  const int tid = threadIdx.x, chunk = (N + LT - 1) / LT;
  const int lo = min(tid * chunk, N), hi = min(lo + chunk, N);
  int cnt = 0;
  for (int q = lo; q < hi; ++q) cnt += st.active[q];
  scan[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < LT; off <<= 1) {
    const int add = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int run = scan[tid] - cnt;
  for (int q = lo; q < hi; ++q) {
    st.rank[q] = run;
    run += st.active[q];
  }
  __syncthreads();
  for (int r = tid; r < N; r += LT) labels[r] = st.rank[st.member[r]];
  if (tid == 0) *n_clusters = scan[LT - 1];
}

constexpr int kRepairBlocksStep = 128;

}  // namespace

hipError_t launch_ahc_init(const float* S, int64_t N, int64_t lds, const AhcState& st, hipStream_t s) {
  const unsigned nb = (unsigned)((N + 31) / 32);
  hipLaunchKernelGGL(ahc_convert_kernel, dim3(nb, nb), dim3(32, 8), 0, s, S, (long long)N, (long long)lds, st.A);
  hipLaunchKernelGGL(ahc_state_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, st, (int)N);
  hipLaunchKernelGGL(ahc_repair_kernel, dim3((unsigned)std::min<int64_t>(N, 4096)), dim3(RT), 0, s, st, (int)N);
  return hipGetLastError();
}

hipError_t launch_ahc_steps(int64_t N, float threshold, const AhcState& st, int steps, hipStream_t s) {
  const unsigned mb = (unsigned)((N + 255) / 256);
  const unsigned rb = (unsigned)std::min<int64_t>(N, kRepairBlocksStep);
  for (int t = 0; t < steps; ++t) {
    hipLaunchKernelGGL(ahc_select_kernel, dim3(1), dim3(ST), 0, s, st, (int)N, (double)threshold);
    hipLaunchKernelGGL(ahc_merge_kernel, dim3(mb), dim3(256), 0, s, st, (int)N);
    hipLaunchKernelGGL(ahc_repair_kernel, dim3(rb), dim3(RT), 0, s, st, (int)N);
  }
  return hipGetLastError();
}

hipError_t launch_ahc_labels(int64_t N, const AhcState& st, int32_t* labels, int32_t* n_clusters, hipStream_t s) {
  hipLaunchKernelGGL(ahc_labels_kernel, dim3(1), dim3(LT), 0, s, st, (int)N, labels, n_clusters);
  return hipGetLastError();
}

}  // namespace spk
