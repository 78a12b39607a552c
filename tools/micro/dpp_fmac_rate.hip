// Microbenchmark: what a row broadcast folded into its multiply-add costs on gfx950, for one wavefront alone on its SIMD
// (the tree solver of the latency IK kernel).  Per update acc -= bcast_row(l, k) * l:
//   (a) v_mov_b64_dpp + v_fma_f64, the pair the compiler emits for row_bcast_d + fma
//   (b) v_fmac_f64_dpp, the folded form (row_bcast_fma and its multi-update forms in csrc/gmr_device_math.h)
//   (c) plain v_fmac_f64, no broadcast: the floor
// each as ONE dependent chain (16 updates of one accumulator) and as eight independent accumulators (2 x 8 updates), and
// one step of a back substitution, where the chain runs through the DPP source (multiply, 2 wait states, update).
// hipcc --offload-arch=gfx950 -O3 dpp_fmac_rate.hip -o dpp_fmac_rate
#include <hip/hip_runtime.h>
#include <cstdio>

#define CTRL " row_newbcast:3 row_mask:0xf bank_mask:0xf"
template <int MODE>
__global__ void k(unsigned long long* out, double* sink, int iters) {
  const int t = threadIdx.x;
  double l = 1e-3 + t * 1e-9, m = 0.999 + t * 1e-9, tmp = 0.0;
  double a0 = 1.0 + t * 1e-9, a1 = 2.0, a2 = 3.0, a3 = 4.0, a4 = 5.0, a5 = 6.0, a6 = 7.0, a7 = 8.0;
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < iters; i++) {
    // dependent chains: 16 updates of a0
    if (MODE == 0) asm volatile(".rept 16\n\tv_mov_b64_dpp %1, %2" CTRL " bound_ctrl:1\n\tv_fma_f64 %0, -%2, %1, %0\n\t.endr" : "+v"(a0), "+v"(tmp) : "v"(l));
    if (MODE == 1) asm volatile(".rept 16\n\tv_fmac_f64_dpp %0, %1, -%1" CTRL "\n\t.endr" : "+v"(a0) : "v"(l));
    if (MODE == 2) asm volatile(".rept 16\n\tv_fmac_f64_e32 %0, %1, %1\n\t.endr" : "+v"(a0) : "v"(l));
    // eight independent accumulators, two updates each
#define EIGHT(LINE) ".rept 2\n\t" LINE("%0") LINE("%1") LINE("%2") LINE("%3") LINE("%4") LINE("%5") LINE("%6") LINE("%7") ".endr"
#define ACCS "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
#define PAIR(A) "v_mov_b64_dpp %8, %9" CTRL " bound_ctrl:1\n\tv_fma_f64 " A ", -%9, %8, " A "\n\t"
#define FOLD(A) "v_fmac_f64_dpp " A ", %8, -%8" CTRL "\n\t"
#define PLAIN(A) "v_fmac_f64_e32 " A ", %8, %8\n\t"
    if (MODE == 3) asm volatile(EIGHT(PAIR) : ACCS, "+v"(tmp) : "v"(l));
    if (MODE == 4) asm volatile(EIGHT(FOLD) : ACCS : "v"(l));
    if (MODE == 5) asm volatile(EIGHT(PLAIN) : ACCS : "v"(l));
    // the statement of one pivot as the solver issues it: s_nop 1 + 14 folded updates (two more accumulators reused)
    if (MODE == 6) asm volatile("s_nop 1\n\t" FOLD("%0") FOLD("%1") FOLD("%2") FOLD("%3") FOLD("%4") FOLD("%5") FOLD("%6") FOLD("%7")
                                FOLD("%0") FOLD("%1") FOLD("%2") FOLD("%3") FOLD("%4") FOLD("%5") FOLD("%0") FOLD("%1") : ACCS : "v"(l));
    // back substitution, 16 steps: x = bcast(a0 * m, k); a0 -= l * x  -- the chain runs through the DPP source
    if (MODE == 7) asm volatile(".rept 16\n\tv_mul_f64 %1, %0, %3\n\ts_nop 1\n\tv_mov_b64_dpp %1, %1" CTRL " bound_ctrl:1\n\tv_fma_f64 %0, -%2, %1, %0\n\t.endr"
                                : "+v"(a0), "+v"(tmp) : "v"(l), "v"(m));
    if (MODE == 8) asm volatile(".rept 16\n\tv_mul_f64 %1, %0, %3\n\ts_nop 1\n\tv_fmac_f64_dpp %0, %1, -%2" CTRL "\n\t.endr"
                                : "+v"(a0), "+v"(tmp) : "v"(l), "v"(m));
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (t == 0) out[blockIdx.x] = t1 - t0;
  sink[blockIdx.x * blockDim.x + t] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + tmp;
}

int main() {
  unsigned long long* d; double* s;
  if (hipMalloc(&d, 64 * 8) != hipSuccess || hipMalloc(&s, 64 * 256 * 8) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  const char* names[] = {"(a) mov_dpp + fma, one dependent chain", "(b) fmac_dpp, one dependent chain", "(c) fmac, one dependent chain",
                         "(a) mov_dpp + fma, 8 independent accumulators", "(b) fmac_dpp, 8 independent accumulators",
                         "(c) fmac, 8 independent accumulators", "(b) s_nop 1 + 16 fmac_dpp (one pivot's statement)",
                         "back substitution step: mul, s_nop 1, mov_dpp, fma", "back substitution step: mul, s_nop 1, fmac_dpp"};
  const int iters = 2000;
  for (int nw : {1, 4}) {
    for (int m = 0; m < 9; m++) {
      switch (m) {
        case 0: hipLaunchKernelGGL(k<0>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 1: hipLaunchKernelGGL(k<1>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 2: hipLaunchKernelGGL(k<2>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 3: hipLaunchKernelGGL(k<3>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 4: hipLaunchKernelGGL(k<4>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 5: hipLaunchKernelGGL(k<5>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 6: hipLaunchKernelGGL(k<6>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 7: hipLaunchKernelGGL(k<7>, 1, 64 * nw, 0, 0, d, s, iters); break;
        case 8: hipLaunchKernelGGL(k<8>, 1, 64 * nw, 0, 0, d, s, iters); break;
      }
      unsigned long long h = 0;
      if (hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("hipMemcpy failed\n"); return 1; }
      printf("waves=%d  %-52s %7.2f cycles/update\n", nw, names[m], (double)h / (16.0 * iters));
    }
  }
  return 0;
}
