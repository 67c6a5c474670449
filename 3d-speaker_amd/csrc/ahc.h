// Average-linkage AHC on a cosine affinity: workspace layout (host, ahc_abi.cpp) + launchers
// (ahc.hip).
#pragma once
#include "common.h"

namespace spk {

// largest N the library clusters: the fp64 working matrix of N = 32,768 is 8 GiB
constexpr int64_t kAhcMaxN = 32768;
// merge steps enqueued between two host reads of the `done` word
constexpr int kAhcChunkSteps = 256;

// control words (AhcState::ctrl)
enum AhcCtrl : int {
  AHC_RUN = 0,       // the launch gate (SPK_GATE), 1 - done: select clears it when the best pair is
                     // below the threshold or one cluster is left
  AHC_I = 1,         // the pair select chose, i < j; the merged cluster keeps index i
  AHC_J = 2,
  AHC_SI = 3,        // their sizes before the merge
  AHC_SJ = 4,
  AHC_NSTALE = 5,    // entries of `stale`
  AHC_NACTIVE = 6,   // clusters left
  AHC_STEPS = 7,     // merges done
  AHC_CTRL_WORDS = 16,
};

// Everything the loop keeps, carved from the caller's workspace.  A is symmetric (row stride N);
// row r's cache (val[r], col[r]) is the largest A[r][c] over active c > r, smallest c on ties
// (col -1: no active column above r).
struct AhcState {
  double* A = nullptr;     // [N][N]
  double* val = nullptr;   // [N]
  int* col = nullptr;      // [N]
  int* size = nullptr;     // [N] members of cluster r
  int* active = nullptr;   // [N] 1 while r is a cluster
  int* member = nullptr;   // [N] cluster of input row r (= its smallest member)
  int* stale = nullptr;    // [N] rows whose cache the next repair rescans
  int* rank = nullptr;     // [N] epilogue: active clusters below r
  int* ctrl = nullptr;     // [AHC_CTRL_WORDS]
};

inline size_t ahc_workspace_bytes(int64_t N) {
  const size_t n = (size_t)N;
  const size_t b = n * n * sizeof(double) + n * sizeof(double) + 6 * n * sizeof(int) + AHC_CTRL_WORDS * sizeof(int);
  return (b + 255) / 256 * 256;
}

inline AhcState ahc_carve(void* workspace, int64_t N) {
  const size_t n = (size_t)N;
  AhcState s;
  s.A = reinterpret_cast<double*>(workspace);
  s.val = s.A + n * n;
  s.col = reinterpret_cast<int*>(s.val + n);
  s.size = s.col + n;
  s.active = s.size + n;
  s.member = s.active + n;
  s.stale = s.member + n;
  s.rank = s.stale + n;
  s.ctrl = s.rank + n;
  return s;
}

// Not linked into the host-only build of the executor (tests/emu): weak, checked by the ABI.
// init: A = double(upper triangle of S) mirrored, singletons, every row's cache.
hipError_t launch_ahc_init(const float* S, int64_t N, int64_t lds, const AhcState& st, hipStream_t s)
    __attribute__((weak));
// `steps` x (select, merge, repair), each launch gated on the `done` word
hipError_t launch_ahc_steps(int64_t N, float threshold, const AhcState& st, int steps, hipStream_t s)
    __attribute__((weak));
// first-occurrence labels and the cluster count
hipError_t launch_ahc_labels(int64_t N, const AhcState& st, int32_t* labels, int32_t* n_clusters, hipStream_t s)
    __attribute__((weak));

// ---- batched form (ahc_batched.hip): one workgroup per problem runs the whole loop in one launch
// largest N of a batched problem: the workgroup's state is 28 N bytes of LDS (112 KiB of the CU's
// 160 KiB at the cap) and the working matrix 8 N^2 bytes of workspace (128 MiB)
#define SPK_AHC_BATCH_MAX_N 4096
// problems per launch: their descriptors travel as kernel arguments (40 bytes each)
constexpr int kAhcBatchChunk = 64;

struct AhcBatchProb {
  const float* S;     // [N][lds] affinity
  int32_t* labels;    // [N]
  double* A;          // [N][N] working matrix, in the workspace
  long long lds;
  int N;
  float thr;
};

struct AhcBatchArgs {
  AhcBatchProb p[kAhcBatchChunk];
  int32_t* n_clusters;   // [n], this chunk's slice
  int n;
};

inline size_t ahc_batched_matrix_bytes(int64_t N) {
  const size_t n = (size_t)N;
  return (n * n * sizeof(double) + 255) / 256 * 256;
}

// two launches for a.n <= kAhcBatchChunk problems: A = double(upper triangle of S) mirrored for all
// of them, then the loop and the labels, a workgroup per problem
hipError_t launch_ahc_batched(const AhcBatchArgs& a, hipStream_t s) __attribute__((weak));

}  // namespace spk
