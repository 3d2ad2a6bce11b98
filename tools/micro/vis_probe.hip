// Visibility-table gate probe: what does it cost to read two random 128-byte
// records per agent out of a table of 100 MB ... 8.9 GB ("lidar
// marks from a per-cell table")?  2,048 one-wave workgroups, two env slots of
// 32 lanes per wave, 4 agents per slot, 8 lanes of 16 bytes per record -- the
// C2 step kernel's geometry at 4,096 envs.  A lane
//   1. loads its agent's two record indices (the step kernel's round trip 1
//      gives it the robot's cell and target cell),
//   2. issues two 16-byte loads, one into each record (round trip 2),
//   3. stores a word that depends on both.
// Launches run back to back from a captured graph (the method of
// head_probe.hip); launch t reads index table t, and the tables differ by
//   fixed   the same records every launch (everything cache-warm: lower bound)
//   walk1   each agent's record moves by +-1 record per launch (a step in y)
//   walk130 ... by +-130 records (+-16.6 KB: a step in x on a 130-wide grid)
//   walk    either, at random (an agent's real walk)
//   random  fresh random records every launch (upper bound)
// The second candidate of a launch is the first one moved by one more such step.
// `stride` 128 reads 128-byte records; 64 reads the packed 64-byte record (4
// lanes of 16 bytes do the work, the table is half as large).
//   hipcc -O3 --offload-arch=gfx950 -o vis_probe tools/micro/vis_probe.hip
//   ./vis_probe [MB ...]     (default: 100 1000 4400 8900)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

constexpr int kBlocks = 2048, kSlots = 2, kAgents = 4, kLaunches = 200;
constexpr int kIdxPerLaunch = kBlocks * kSlots * kAgents * 2;  // two candidates per agent

__global__ __launch_bounds__(64) void k_vis(const char* __restrict__ tab, const uint32_t* __restrict__ idx,
                                            uint32_t nrec, uint32_t stride, int* __restrict__ q) {
  const uint32_t lane = threadIdx.x, slot = lane >> 5, ag = (lane >> 3) & 3, chunk = lane & 7;
  const uint2 c = *reinterpret_cast<const uint2*>(idx + ((blockIdx.x * kSlots + slot) * kAgents + ag) * 2);
  const uint32_t r0 = c.x < nrec ? c.x : 0u, r1 = c.y < nrec ? c.y : 0u;  // never out of the table
  const uint32_t off = (chunk * 16u) & (stride - 1u);
  const int4 a = *reinterpret_cast<const int4*>(tab + (size_t)r0 * stride + off);
  const int4 b = *reinterpret_cast<const int4*>(tab + (size_t)r1 * stride + off);
  q[blockIdx.x * 64 + lane] = a.x + a.w + b.y + b.z + 1;
}
// the same without the table: what the kernel boundary, the index load and the store cost
__global__ __launch_bounds__(64) void k_base(const uint32_t* __restrict__ idx, int* __restrict__ q) {
  const uint32_t lane = threadIdx.x, slot = lane >> 5, ag = (lane >> 3) & 3;
  const uint2 c = *reinterpret_cast<const uint2*>(idx + ((blockIdx.x * kSlots + slot) * kAgents + ag) * 2);
  q[blockIdx.x * 64 + lane] = (int)((c.x ^ c.y) & 1u) + 1;
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <typename F>
static float timeit(F launch, hipStream_t st) {
  hipGraph_t g; hipGraphExec_t ge;
  hipStreamBeginCapture(st, hipStreamCaptureModeGlobal);
  for (int t = 0; t < kLaunches; ++t) launch(t);
  hipStreamEndCapture(st, &g);
  hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  hipGraphLaunch(ge, st); hipStreamSynchronize(st);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    hipEventRecord(e0, st); hipGraphLaunch(ge, st); hipEventRecord(e1, st);
    hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  hipGraphExecDestroy(ge); hipGraphDestroy(g);
  return best * 1000.f / kLaunches;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

enum Mode { FIXED, WALK1, WALK130, WALK, RANDOM, NMODES };
static const char* kModeName[NMODES] = {"fixed", "walk1", "walk130", "walk", "random"};

static uint32_t moved(uint32_t r, uint32_t nrec, Mode m) {
  const uint32_t v = rnd();
  const int64_t d = (m == WALK1 || (m == WALK && (v & 2))) ? 1 : 130;
  const int64_t n = (int64_t)r + ((v & 1) ? d : -d);
  return n < 0 || n >= (int64_t)nrec ? r : (uint32_t)n;
}

int main(int argc, char** argv) {
  std::vector<long> mbs;
  for (int i = 1; i < argc; ++i) mbs.push_back(atol(argv[i]));
  if (mbs.empty()) mbs = {100, 1000, 4400, 8900};
  hipStream_t st; CK(hipStreamCreate(&st));
  int* q; CK(hipMalloc(&q, kBlocks * 64 * sizeof(int)));
  uint32_t* idx; CK(hipMalloc(&idx, (size_t)kLaunches * kIdxPerLaunch * 4));
  std::vector<uint32_t> h((size_t)kLaunches * kIdxPerLaunch);
  int bad = 0;
  for (long mb : mbs) {
    for (uint32_t stride : {128u, 64u}) {
      const size_t nrec64 = (size_t)mb * 1000000 / 128;  // records: the 64-byte table is half the bytes
      if (nrec64 < 1024 || nrec64 > 0xFFFFFFFFull) { printf("skip %ld MB\n", mb); continue; }
      const uint32_t nrec = (uint32_t)nrec64;
      char* tab; CK(hipMalloc(&tab, (size_t)nrec * stride));
      CK(hipMemset(tab, 0, (size_t)nrec * stride));
      for (int m = 0; m < NMODES; ++m) {
        for (size_t i = 0; i < (size_t)kIdxPerLaunch; i += 2) {
          h[i] = rnd() % nrec;
          h[i + 1] = m == FIXED || m == RANDOM ? rnd() % nrec : moved(h[i], nrec, (Mode)m);
        }
        for (int t = 1; t < kLaunches; ++t)
          for (size_t i = 0; i < (size_t)kIdxPerLaunch; i += 2) {
            const size_t o = (size_t)t * kIdxPerLaunch + i, p = o - kIdxPerLaunch;
            if (m == FIXED) { h[o] = h[p]; h[o + 1] = h[p + 1]; }
            else if (m == RANDOM) { h[o] = rnd() % nrec; h[o + 1] = rnd() % nrec; }
            else { h[o] = (rnd() & 1) ? h[p + 1] : h[p]; h[o + 1] = moved(h[o], nrec, (Mode)m); }  // moved or blocked
          }
        CK(hipMemcpy(idx, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        const float base = timeit([&](int t) {
          hipLaunchKernelGGL(k_base, dim3(kBlocks), dim3(64), 0, st, (const uint32_t*)idx + (size_t)t * kIdxPerLaunch, q); }, st);
        const float tv = timeit([&](int t) {
          hipLaunchKernelGGL(k_vis, dim3(kBlocks), dim3(64), 0, st, (const char*)tab,
                             (const uint32_t*)idx + (size_t)t * kIdxPerLaunch, nrec, stride, q); }, st);
        printf("table %5ld MB-equiv  record %3u B  (%7.1f MB)  %-8s base %.3f us  table %.3f us  (+%.3f)\n", mb, stride,
               (double)nrec * stride / 1e6, kModeName[m], base, tv, tv - base);
        fflush(stdout);
      }
      CK(hipStreamSynchronize(st));
      int out = 0; CK(hipMemcpy(&out, q + kBlocks * 64 - 1, 4, hipMemcpyDeviceToHost));
      if (out != 1) { printf("check: q[last] = %d (expect 1)\n", out); bad = 1; }
      CK(hipFree(tab));
    }
  }
  return bad ? 2 : 0;
}
