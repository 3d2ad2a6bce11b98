// Fused-steps gate probe: what does a kernel boundary per step cost a wave
// whose step re-reads what it wrote one step earlier ("Fused
// steps")?  2,048 one-wave workgroups -- the C2 step kernel's geometry at
// 4,096 envs.  Per step t a lane
//   1. loads its index word (the step kernel's action bytes),
//   2. loads 16 bytes of the wave's state at that index, and 16 more at an
//      index taken from the first (two dependent loads; the same wave stored
//      both one step earlier),
//   3. loads its word of the wave's "union" line (the target of step t-1's ORs),
//   4. stores 16 bytes of new state,
//   5. ORs a bit into a neighbour lane's word of the union line (returning-free
//      atomic, executed at L2), which that lane reads in step t+1.
// Variant (a): 200 launches of one step each, back to back from a captured
// graph (the method of head_probe.hip).  Variant (b): one launch that loops 200
// steps with a workgroup-scope release / acquire fence at the loop bottom --
// the ordering the env kernel's step loop uses.  Both run the same kernel.
// The probe checks itself: after all steps every state word and every union
// word must equal what a host loop computes, so a read served from a stale
// cache line shows as a wrong value.
//   hipcc -O3 --offload-arch=gfx950 -o loop_probe tools/micro/loop_probe.hip
//   ./loop_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

constexpr int kBlocks = 2048, kSteps = 200, kIdxPeriod = 8, kRuns = 6;  // 1 warm-up + 5 timed runs of kSteps
constexpr int kLanes = kBlocks * 64;

struct U4 { uint32_t x, y, z, w; };

// one lane's step: the new state from the two loaded states, the union word and t
__host__ __device__ inline U4 next_state(const U4& a, const U4& b, uint32_t v, uint32_t t) {
  U4 n;
  n.x = a.x * 1664525u + b.y + v + t;
  n.y = a.y ^ (b.z + 0x9E3779B9u);
  n.z = a.z + b.w * 3u + (v >> 7);
  n.w = (a.w ^ b.x) + 1u;
  return n;
}

// steps t0 .. t0 + n - 1; state planes alternate (step t reads plane t & 1)
__global__ __launch_bounds__(64) void k_steps(const uint32_t* __restrict__ idx, U4* st, uint32_t* un, int t0, int n) {
  const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u;
  for (int t = t0; t < t0 + n; ++t) {
    const uint32_t i0 = idx[(t % kIdxPeriod) * kLanes + base + lane] & 63u;
    const U4* rd = st + (size_t)(t & 1) * kLanes + base;
    U4* wr = st + (size_t)((t + 1) & 1) * kLanes + base;
    const U4 a = rd[i0];
    const U4 b = rd[a.x & 63u];
    const uint32_t v = un[base + lane];
    const U4 nw = next_state(a, b, v, (uint32_t)t);
    wr[lane] = nw;
    atomicOr(&un[base + ((lane + 1u) & 63u)], 1u << ((nw.x ^ (uint32_t)t) & 31u));  // (depends on v: after the load)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

// kRuns runs of kSteps steps, `per` steps per launch; us per step, best of the timed runs
static float timeit(int per, const uint32_t* idx, U4* st, uint32_t* un, hipStream_t s) {
  hipGraph_t g; hipGraphExec_t ge;
  hipStreamBeginCapture(s, hipStreamCaptureModeGlobal);
  for (int t = 0; t < kSteps; t += per) hipLaunchKernelGGL(k_steps, dim3(kBlocks), dim3(64), 0, s, idx, st, un, t, per);
  hipStreamEndCapture(s, &g);
  hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  hipGraphLaunch(ge, s); hipStreamSynchronize(s);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e30f;
  for (int rep = 1; rep < kRuns; ++rep) {
    hipEventRecord(e0, s); hipGraphLaunch(ge, s); hipEventRecord(e1, s);
    hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  hipGraphExecDestroy(ge); hipGraphDestroy(g);
  return best * 1000.f / kSteps;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main() {
  std::vector<uint32_t> hidx((size_t)kIdxPeriod * kLanes), hun0(kLanes, 0u);
  std::vector<U4> hst0((size_t)2 * kLanes);
  for (auto& v : hidx) v = rnd();
  for (auto& v : hst0) v = U4{rnd(), rnd(), rnd(), rnd()};
  // the host loop: kRuns * kSteps steps from the initial state
  std::vector<U4> est = hst0;
  std::vector<uint32_t> eun = hun0, orv(64);
  for (int run = 0; run < kRuns; ++run)
    for (int t = 0; t < kSteps; ++t)
      for (int w = 0; w < kBlocks; ++w) {
        const size_t base = (size_t)w * 64;
        const U4* rd = est.data() + (size_t)(t & 1) * kLanes + base;
        U4* wr = est.data() + (size_t)((t + 1) & 1) * kLanes + base;
        for (uint32_t l = 0; l < 64; ++l) {
          const uint32_t i0 = hidx[(size_t)(t % kIdxPeriod) * kLanes + base + l] & 63u;
          const U4 a = rd[i0], b = rd[a.x & 63u];
          const U4 nw = next_state(a, b, eun[base + l], (uint32_t)t);
          wr[l] = nw;
          orv[(l + 1u) & 63u] = 1u << ((nw.x ^ (uint32_t)t) & 31u);
        }
        for (uint32_t l = 0; l < 64; ++l) eun[base + l] |= orv[l];
      }

  hipStream_t s; CK(hipStreamCreate(&s));
  uint32_t *idx, *un; U4* st;
  CK(hipMalloc(&idx, hidx.size() * 4));
  CK(hipMalloc(&st, hst0.size() * sizeof(U4)));
  CK(hipMalloc(&un, hun0.size() * 4));
  CK(hipMemcpy(idx, hidx.data(), hidx.size() * 4, hipMemcpyHostToDevice));
  std::vector<U4> gst(hst0.size());
  std::vector<uint32_t> gun(hun0.size());
  int bad = 0;
  float us[2] = {0.f, 0.f};
  const int per[2] = {1, kSteps};
  for (int v = 0; v < 2; ++v) {
    CK(hipMemcpy(st, hst0.data(), hst0.size() * sizeof(U4), hipMemcpyHostToDevice));
    CK(hipMemcpy(un, hun0.data(), hun0.size() * 4, hipMemcpyHostToDevice));
    us[v] = timeit(per[v], idx, st, un, s);
    CK(hipStreamSynchronize(s));
    CK(hipMemcpy(gst.data(), st, gst.size() * sizeof(U4), hipMemcpyDeviceToHost));
    CK(hipMemcpy(gun.data(), un, gun.size() * 4, hipMemcpyDeviceToHost));
    size_t wrong = 0;
    for (size_t i = 0; i < gst.size(); ++i)
      wrong += gst[i].x != est[i].x || gst[i].y != est[i].y || gst[i].z != est[i].z || gst[i].w != est[i].w;
    for (size_t i = 0; i < gun.size(); ++i) wrong += gun[i] != eun[i];
    printf("variant (%c) %3d step(s) per launch, %3d launches: %.3f us per step (best of %d)  check: %zu wrong words of %zu\n",
           v ? 'b' : 'a', per[v], kSteps / per[v], us[v], kRuns - 1, wrong, gst.size() + gun.size());
    fflush(stdout);
    if (wrong) bad = 1;
  }
  printf("(a) - (b) = %.3f us per step\n", us[0] - us[1]);
  return bad ? 2 : 0;
}
