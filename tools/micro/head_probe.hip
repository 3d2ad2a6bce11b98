// Kernel-head probe: 2,048 one-wave workgroups, each one dependent global
// load and one store, launched back to back from a captured graph (the
// method of kernarg_probe.hip).  The pointer comes
//   (a) out of a ~700-byte by-value struct (like the env kernel's EnvArgs:
//       the compiler must s_load it before any vector load can issue), or
//   (b) as a leading scalar parameter in front of the same struct, which
//       gfx950 can preload into SGPRs at wave launch when this file is built
//       with  -mllvm -amdgpu-kernarg-preload-count=6 .
// Build it twice, with and without the flag: (b) with the flag against (b)
// without it is what kernarg preloading gains on this firmware; (a) is the
// same in both builds (a by-value struct is never preloaded).
//   hipcc -O3 --offload-arch=gfx950 [-mllvm -amdgpu-kernarg-preload-count=6] \
//         -o head_probe tools/micro/head_probe.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

struct Big {
  int ints[45];     // ~180 bytes of ints in front of the pointers
  const int* p;
  int* q;
  int64_t tail[62];  // ~700 bytes in all
};

__global__ __launch_bounds__(64) void k_struct(Big b) {
  if (threadIdx.x == 0) b.q[blockIdx.x] = b.p[blockIdx.x] + b.ints[44] + (int)b.tail[61];
}
__global__ __launch_bounds__(64) void k_head(const int* p, int* q, int n, Big b) {
  if (threadIdx.x == 0) {
    const int v = p[blockIdx.x < n ? blockIdx.x : 0];  // address from the head alone
    q[blockIdx.x] = v + b.ints[44] + (int)b.tail[61];
  }
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <typename F>
static float timeit(F launch, hipStream_t st, int n) {
  hipGraph_t g; hipGraphExec_t ge;
  hipStreamBeginCapture(st, hipStreamCaptureModeGlobal);
  for (int i = 0; i < n; ++i) launch();
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
  hipGraphExecDestroy(ge); hipGraphDestroy(g);
  return best * 1000.f / n;
}

int main() {
  hipStream_t st; CK(hipStreamCreate(&st));
  const int blocks = 2048, n = 500;
  int *p, *q; CK(hipMalloc(&p, blocks * 4)); CK(hipMalloc(&q, blocks * 4)); CK(hipMemset(p, 0, blocks * 4));
  Big b = {}; b.p = p; b.q = q; b.ints[44] = 2; b.tail[61] = 1;
  for (int rep = 0; rep < 3; ++rep) {
    const float a = timeit([&] { hipLaunchKernelGGL(k_struct, dim3(blocks), dim3(64), 0, st, b); }, st, n);
    const float h = timeit([&] { hipLaunchKernelGGL(k_head, dim3(blocks), dim3(64), 0, st, (const int*)p, q, blocks, b); }, st, n);
    printf("rep %d: (a) pointer in the struct %.3f us, (b) pointer in the head %.3f us per launch\n", rep, a, h);
  }
  CK(hipStreamSynchronize(st));
  int out = 0; CK(hipMemcpy(&out, q + blocks - 1, 4, hipMemcpyDeviceToHost));
  printf("check: q[last] = %d (expect 3)\n", out);
  return out == 3 ? 0 : 2;
}
