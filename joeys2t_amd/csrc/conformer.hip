// Conformer convolution-module kernels (reference transformer_layers.py:410-475): depthwise convolution along the OUTER
// index of an [L, N, C] array (the reference's module convolves over the batch index, see the header) and BatchNorm1d
// over the rows of [rows, C] fused with the activation that follows it.  All HBM-bound element-wise / column-reduction
// work: f32 arithmetic, bf16 or f32 storage, channel index fastest (coalesced).
#include "common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------- depthwise conv
constexpr int DW_MAXK = 63;
#define DISPATCH_DT(dt, T, ...)                                   \
  if ((dt) == JS2T_F32) { using T = float; __VA_ARGS__; }         \
  else { using T = uint16_t; __VA_ARGS__; }


template <typename T>
__global__ __launch_bounds__(256) void dwconv_outer_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, T* __restrict__ y, int64_t L,
                                                               int64_t N, int64_t C, int K) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L * N * C) return;
  const int64_t c = i % C, ln = i / C, n = ln % N, l = ln / N;
  const int pad = (K - 1) / 2;
  float acc = bias ? bias[c] : 0.f;
  for (int k = 0; k < K; ++k) {
    const int64_t ls = l + k - pad;
    if (ls >= 0 && ls < L) acc += w[c * K + k] * io<T>::ld(x + (ls * N + n) * C + c);
  }
  io<T>::st(y + i, acc);
}

// The same convolution for bf16 with C % 128 == 0 and L <= 64 (L is the BATCH size here, see the header): a block stages
// the slab x[0..L, 4 n, 128 c] (at most 64 KB) and the 128 channels' taps in LDS; a thread then owns one channel PAIR of one
// n for every l - its reads walk consecutive 4-byte LDS words (conflict-free), every global byte is read exactly once in
// 256-byte runs.  The one-output-per-thread kernel above issues 31 scattered 2-byte loads and 31 strided tap loads per
// output and ran at 2 % of the HBM rate (322 us for 12 MB at L = 32, K = 31).  FLIP: taps reversed (input gradient).
template <bool FLIP>
__global__ __launch_bounds__(256) void dwconv_outer_lds_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, uint16_t* __restrict__ y, int L, int64_t N,
                                                               int64_t C, int K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  uint32_t* xs = (uint32_t*)dsm;                    // [L][4][64] channel pairs
  float2* ws = (float2*)(dsm + (size_t)L * 1024);  // [K][64] taps of the pair
  const int t = threadIdx.x, cp = t & 63, nn = t >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 128, n = (int64_t)blockIdx.y * 4 + nn;
  const bool live = n < N;
  for (int l = 0; l < L; ++l)
    xs[(l * 4 + nn) * 64 + cp] = live ? *(const uint32_t*)(x + ((int64_t)l * N + n) * C + c0 + 2 * cp) : 0u;
  for (int i = t; i < K * 64; i += 256) {
    const int k = i >> 6, p = i & 63;
    ws[i] = make_float2(w[(c0 + 2 * p) * K + k], w[(c0 + 2 * p + 1) * K + k]);
  }
  __syncthreads();
  if (!live) return;
  const int pad = (K - 1) / 2;
  const float b0 = bias ? bias[c0 + 2 * cp] : 0.f, b1 = bias ? bias[c0 + 2 * cp + 1] : 0.f;
  for (int lb = 0; lb < L; lb += 8) {
    float a0[8], a1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a0[j] = b0, a1[j] = b1;
    for (int k = 0; k < K; ++k) {
      const float2 wk = ws[k * 64 + cp];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int li = FLIP ? lb + j - k + pad : lb + j + k - pad;
        const uint32_t v = xs[(min(max(li, 0), L - 1) * 4 + nn) * 64 + cp];
        const bool in = li >= 0 && li < L;
        a0[j] = fmaf(wk.x, in ? __uint_as_float(v << 16) : 0.f, a0[j]);
        a1[j] = fmaf(wk.y, in ? __uint_as_float(v & 0xffff0000u) : 0.f, a1[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (lb + j < L)
        *(uint32_t*)(y + ((int64_t)(lb + j) * N + n) * C + c0 + 2 * cp) =
            pack_bf16x2(a0[j], a1[j]);
  }
}
template <bool FLIP>
bool dwconv_outer_lds_launch(const void* x, const float* w, const float* bias, void* y, int64_t L, int64_t N, int64_t C, int K, int dt,
                             hipStream_t s) {
  if (dt != JS2T_BF16 || (C & 127) || L > 64 || L < 1 || ((((uintptr_t)x) | ((uintptr_t)y)) & 3) || (N + 3) / 4 > 65535) return false;
  const size_t lds = (size_t)L * 1024 + (size_t)K * 64 * sizeof(float2);
  // (JS2T_LDS_ONCE written out: a failure is no error here, the caller falls back to its plain kernel)
  static const hipError_t lds_e = js2t_lds_optin_raw((const void*)dwconv_outer_lds_kernel<FLIP>, 64 * 1024 + 63 * 512);
  if (lds_e != hipSuccess) return false;
  hipLaunchKernelGGL(dwconv_outer_lds_kernel<FLIP>, dim3((unsigned)(C / 128), (unsigned)((N + 3) / 4)), dim3(256), lds, s,
                     (const uint16_t*)x, w, bias, (uint16_t*)y, (int)L, N, C, K);
  return true;
}

// The same convolution from REGISTER windows (round 4): a thread owns one (n, c) column, keeps the channel's K taps and a
// window of LC + KM - 1 inputs along l in registers and writes LC outputs per window - every input loaded once per window
// (1 + (K-1)/LC times overall), no LDS, no barrier, any dtype / channel count.  FLIP: taps reversed (input gradient; the
// reversed taps are loaded in reversed order, so the sum runs over k descending).  52 -> ~15 us at L = 32, N = 375, C = 512.
template <typename T, int KM, int LC, bool FLIP>
__global__ __launch_bounds__(256) void dwconv_outer_win_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, T* __restrict__ y, int L, int64_t N,
                                                               int64_t C, int K, int n_per_block) {
  const int cl = threadIdx.x & 63, nl = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  if (c >= C) return;
  const int64_t n0 = (int64_t)blockIdx.y * n_per_block, n1 = min(n0 + n_per_block, N);
  const int pad = (K - 1) / 2;
  float wr[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) wr[k] = k < K ? w[c * K + (FLIP ? K - 1 - k : k)] : 0.f;
  const float b = bias ? bias[c] : 0.f;
  const int64_t NC = N * C;
  for (int64_t n = n0 + nl; n < n1; n += 4) {
    const int off = (int)(n * C + c);  // this thread's column inside a row l (N * C < 2^30: checked by the launcher)
    for (int l0 = 0; l0 < L; l0 += LC) {
      float xr[LC + KM - 1];
#pragma unroll
      for (int i = 0; i < LC + KM - 1; ++i) {  // xr[i] = x[l0 + i - pad] (zero outside the sequence)
        // Every load is issued - from a clamped row where the window leaves the sequence - and zeroed by a select (as
        // `cond ? load : 0` each of the 46 loads was a basic block of its own), and its address is a wave-uniform row base
        // plus the thread's 32-bit column offset: formed per load as ((l * N + n) * C + c) in 64 bits the address arithmetic
        // was half of the loop's vector instructions.
        const int ls = l0 + i - pad;
        const T* row = x + (int64_t)min(max(ls, 0), L - 1) * NC;
        const float v = io<T>::ld(row + off);
        xr[i] = (i < LC + K - 1 && ls >= 0 && ls < L) ? v : 0.f;
      }
      if (l0 + LC <= L) {  // whole chunk (wave-uniform): no test per store, one basic block for the 16 outputs
#pragma unroll
        for (int j = 0; j < LC; ++j) {
          float acc = b;
#pragma unroll
          for (int k = 0; k < KM; ++k) acc = fmaf(wr[k], xr[j + k], acc);
          io<T>::st(y + (int64_t)(l0 + j) * NC + off, acc);
        }
      } else {
#pragma unroll
        for (int j = 0; j < LC; ++j) {
          float acc = b;
#pragma unroll
          for (int k = 0; k < KM; ++k) acc = fmaf(wr[k], xr[j + k], acc);
          if (l0 + j < L) io<T>::st(y + (int64_t)(l0 + j) * NC + off, acc);
        }
      }
    }
  }
}
template <bool FLIP>
bool dwconv_outer_win_launch(const void* x, const float* w, const float* bias, void* y, int64_t L, int64_t N, int64_t C, int K, int dt,
                             hipStream_t s) {
  if (K > 31 || L >= 65536 || L < 1 || N * C >= (int64_t(1) << 30)) return false;
  int npb = (int)cdiv(N * cdiv(C, 64), 1024);  // columns per block: about four blocks per CU
  npb = npb < 4 ? 4 : (npb + 3) & ~3;
  if (cdiv(N, npb) > 65535) return false;
  const dim3 grid((unsigned)cdiv(C, 64), (unsigned)cdiv(N, npb));
  if (K <= 15) {
    DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_win_kernel<T, 15, 16, FLIP>), grid, dim3(256), 0, s, (const T*)x, w, bias, (T*)y, (int)L,
                                          N, C, K, npb));
  } else {
    DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_win_kernel<T, 31, 16, FLIP>), grid, dim3(256), 0, s, (const T*)x, w, bias, (T*)y, (int)L,
                                          N, C, K, npb));
  }
  return true;
}

// dx[l,n,c] = sum_k w[c,k] * dy[l - k + pad, n, c]
template <typename T>
__global__ __launch_bounds__(256) void dwconv_outer_dx_kernel(const T* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
                                                              int64_t L, int64_t N, int64_t C, int K) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L * N * C) return;
  const int64_t c = i % C, ln = i / C, n = ln % N, l = ln / N;
  const int pad = (K - 1) / 2;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    const int64_t ls = l - k + pad;
    if (ls >= 0 && ls < L) acc += w[c * K + k] * io<T>::ld(dy + (ls * N + n) * C + c);
  }
  io<T>::st(dx + i, acc);
}

// dw[c,k] += sum_{l,n} dy[l,n,c] * x[l+k-pad,n,c]: block = 64 channels x 4 n-lanes over a slab of n; K accumulators per
// thread, combined over the 4 lanes in LDS, one atomic per (c,k) and block
constexpr int DW_SLAB = 32;
template <typename T>
__global__ __launch_bounds__(256) void dwconv_outer_dw_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ dw,
                                                              int64_t L, int64_t N, int64_t C, int K) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, nl = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  const int64_t n0 = (int64_t)blockIdx.y * DW_SLAB;
  const int pad = (K - 1) / 2;
  float acc[DW_MAXK];
#pragma unroll
  for (int k = 0; k < DW_MAXK; ++k) acc[k] = 0.f;
  if (c < C) {
    for (int64_t n = n0 + nl; n < min(n0 + DW_SLAB, N); n += 4)
      for (int64_t l = 0; l < L; ++l) {
        const float g = io<T>::ld(dy + (l * N + n) * C + c);
#pragma unroll
        for (int k = 0; k < DW_MAXK; ++k) {
          if (k < K) {
            const int64_t ls = l + k - pad;
            if (ls >= 0 && ls < L) acc[k] += g * io<T>::ld(x + (ls * N + n) * C + c);
          }
        }
      }
  }
  typedef __attribute__((address_space(1))) float gfloat;
  for (int k = 0; k < K; ++k) {
    float v = 0.f;
#pragma unroll
    for (int kk = 0; kk < DW_MAXK; ++kk)
      if (kk == k) v = acc[kk];
    red[nl][cl] = v;
    __syncthreads();
    if (nl == 0 && c < C) {
      const float tot = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
      __builtin_amdgcn_global_atomic_fadd_f32((gfloat*)dw + c * K + k, tot);
    }
    __syncthreads();
  }
}

// The same sums with every operand loaded ONCE: a thread owns one (n, c) column, holds a window of LC + KM - 1 values of x and
// LC of dy along l in registers and forms all K lags from them (the kernel above fetches x K times per dy element and runs 96
// blocks at L = 32, N = 375, C = 512: 1.06 ms per Conformer layer, a third of the config-5 train step).  Block = 64 channels x
// 4 columns at a time over a slab of n; lags combined over the four waves in LDS, one atomic per (c, k) and block.
// `part` != nullptr: the block's sums go to part[blockIdx.y][c][k] with plain stores and dwconv_dw_reduce_kernel adds the slabs up in
// order - the 47 atomics per (c, k) of the other form (746 k on 15.9 k addresses at L = 32, N = 375, C = 512) were HALF of this
// kernel's time (68 -> 37 us without them), and the order of the additions is then fixed (deterministic mode needs no special grid).
template <typename T, int KM, int LC>
__global__ __launch_bounds__(256) void dwconv_outer_dw_win_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ dw,
                                                                  int L, int64_t N, int64_t C, int K, int n_per_block,
                                                                  float* __restrict__ part) {
  __shared__ float red[4][KM][64];
  const int cl = threadIdx.x & 63, nl = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  const int64_t n0 = (int64_t)blockIdx.y * n_per_block, n1 = min(n0 + n_per_block, N);
  const int pad = (K - 1) / 2;
  float acc[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) acc[k] = 0.f;
  if (c < C) {
    const int64_t NC = N * C;
    for (int64_t n = n0 + nl; n < n1; n += 4) {
      const int off = (int)(n * C + c);  // (N * C < 2^30: checked by the launcher)
      for (int l0 = 0; l0 < L; l0 += LC) {
        float xr[LC + KM - 1];
#pragma unroll
        for (int i = 0; i < LC + KM - 1; ++i) {  // xr[i] = x[l0 + i - pad] (zero outside the sequence)
          const int ls = l0 + i - pad;  // (unconditional loads from clamped, wave-uniform rows + selects: see dwconv_outer_win_kernel)
          const float v = io<T>::ld(x + (int64_t)min(max(ls, 0), L - 1) * NC + off);
          xr[i] = (i < LC + K - 1 && ls >= 0 && ls < L) ? v : 0.f;
        }
#pragma unroll
        for (int j = 0; j < LC; ++j) {
          const float gv = io<T>::ld(dy + (int64_t)min(l0 + j, L - 1) * NC + off);
          const float g = l0 + j < L ? gv : 0.f;
#pragma unroll
          for (int k = 0; k < KM; ++k) acc[k] = fmaf(g, xr[j + k], acc[k]);  // x[l + k - pad] = xr[(l - l0) + k]
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KM; ++k) red[nl][k][cl] = acc[k];
  __syncthreads();
  typedef __attribute__((address_space(1))) float gfloat;
  if (part) {  // contiguous run of 64 x K floats per block: thread i writes element i (channel i / K, lag i % K)
    float* pb = part + ((int64_t)blockIdx.y * C + (int64_t)blockIdx.x * 64) * K;
    for (int i = threadIdx.x; i < K * 64; i += 256) {
      const int cc = i / K, k = i - cc * K;
      if ((int64_t)blockIdx.x * 64 + cc < C) pb[i] = (red[0][k][cc] + red[1][k][cc]) + (red[2][k][cc] + red[3][k][cc]);
    }
    return;
  }
  for (int i = threadIdx.x; i < K * 64; i += 256) {
    const int k = i >> 6, cc = i & 63;
    const int64_t co = (int64_t)blockIdx.x * 64 + cc;
    if (co < C)
      __builtin_amdgcn_global_atomic_fadd_f32((gfloat*)dw + co * K + k, (red[0][k][cc] + red[1][k][cc]) + (red[2][k][cc] + red[3][k][cc]));
  }
}
// dw[i] += part[0][i] + part[1][i] + ... (slabs in order)
__global__ __launch_bounds__(256) void dwconv_dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int64_t n, int slabs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
  for (int sidx = 0; sidx < slabs; ++sidx) a += part[(int64_t)sidx * n + i];
  dw[i] += a;
}
// Library-owned scratch for the slab sums: allocated ONCE, at the first call (an eager call: hipMalloc is not capturable, and a buffer
// that moved later would leave captured graphs with a dangling pointer), never grown; a call that needs more takes the atomic form.
float* dw_partial_scratch(size_t n_floats) {
  static float* buf = nullptr;
  static size_t cap = 0;
  static bool tried = false;
  if (!tried) {
    tried = true;
    const size_t want = n_floats < (size_t(4) << 20) ? (size_t(4) << 20) : n_floats;  // >= 16 MB: 256 slabs of a 512 x 31 weight
    if (hipMalloc(&buf, want * sizeof(float)) == hipSuccess) cap = want;
    else buf = nullptr;
  }
  return n_floats <= cap ? buf : nullptr;
}

// ---------------------------------------------------------------------------------------------- batch norm + activation
// column reductions over a row slab: MODE 0: (sum x, -) ; 1: (sum (x-mean)^2, -) ; 2: (sum dz, sum dz*xhat) with
// dz = dy * act'(z), z = xhat*gamma + beta.  Block = 64 columns x 4 row lanes; atomics onto out0 / out1 (pre-zeroed).
constexpr int BN_SLAB = 64;
// `slab`: rows per block (BN_SLAB; deterministic mode: all of them - ONE block per 64 columns, so every output receives a single
// sum formed in a fixed order)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_colreduce_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* out0, float* out1, int64_t rows,
                                                           int64_t C, int act, int64_t slab) {
  __shared__ float red[2][4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.y * slab;
  float a0 = 0.f, a1 = 0.f;
  if (c < C) {
    const float mu = MODE >= 1 ? mean[c] : 0.f;
    const float is = MODE == 2 ? invstd[c] : 0.f, ga = MODE == 2 ? gamma[c] : 0.f, be = MODE == 2 ? beta[c] : 0.f;
    for (int64_t r = r0 + rl; r < min(r0 + slab, rows); r += 4) {
      const float v = io<T>::ld(x + r * C + c);
      if (MODE == 0) {
        a0 += v;
      } else if (MODE == 1) {
        a0 += (v - mu) * (v - mu);
      } else {
        const float xh = (v - mu) * is;
        const float dz = io<T>::ld(dy + r * C + c) * (act == JS2T_ACT_NONE ? 1.f : act_grad(xh * ga + be, act));
        a0 += dz;
        a1 += dz * xh;
      }
    }
  }
  red[0][rl][cl] = a0;
  red[1][rl][cl] = a1;
  __syncthreads();
  typedef __attribute__((address_space(1))) float gfloat;
  if (rl == 0 && c < C) {
    __builtin_amdgcn_global_atomic_fadd_f32((gfloat*)out0 + c, (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]));
    if (MODE == 2)
      __builtin_amdgcn_global_atomic_fadd_f32((gfloat*)out1 + c, (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]));
  }
}

__global__ void bn_mean_kernel(const float* sum, float* mean, int64_t rows, int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) mean[c] = sum[c] / (float)rows;
}
// biased variance -> invstd; running statistics (momentum, unbiased variance) as torch.nn.BatchNorm1d
__global__ void bn_finalize_kernel(const float* sqdev, const float* mean, float* invstd, float* running_mean, float* running_var,
                                   int64_t rows, int64_t C, float eps, float momentum) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float var = sqdev[c] / (float)rows;
  invstd[c] = rsqrtf(var + eps);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean[c];
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (sqdev[c] / (float)max((int64_t)1, rows - 1));
}
__global__ void bn_eval_stats_kernel(const float* running_mean, const float* running_var, float* mean, float* invstd, int64_t C,
                                     float eps) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    mean[c] = running_mean[c];
    invstd[c] = rsqrtf(running_var[c] + eps);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_act_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, T* __restrict__ y, int64_t n, int64_t C, int act) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t c = i % C;
  const float z = (io<T>::ld(x + i) - mean[c]) * invstd[c] * gamma[c] + beta[c];
  io<T>::st(y + i, act == JS2T_ACT_NONE ? z : act_apply(z, act));
}

// dx = gamma*invstd*(dz - s0/R - xhat*s1/R)   (train)   |   gamma*invstd*dz   (eval)
template <typename T>
__global__ __launch_bounds__(256) void bn_act_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ s0,
                                                        const float* __restrict__ s1, T* __restrict__ dx, int64_t rows, int64_t C, int act,
                                                        int train) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const int64_t c = i % C;
  const float xh = (io<T>::ld(x + i) - mean[c]) * invstd[c];
  const float dz = io<T>::ld(dy + i) * (act == JS2T_ACT_NONE ? 1.f : act_grad(xh * gamma[c] + beta[c], act));
  const float inv_r = 1.f / (float)rows;
  const float v = train ? dz - s0[c] * inv_r - xh * s1[c] * inv_r : dz;
  io<T>::st(dx + i, gamma[c] * invstd[c] * v);
}
__global__ void bn_param_grad_kernel(const float* s0, const float* s1, float* dgamma, float* dbeta, int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    if (dgamma) dgamma[c] += s1[c];
    if (dbeta) dbeta[c] += s0[c];
  }
}


}  // namespace

extern "C" int js2t_dwconv_outer_fwd(const void* x, const float* w, const float* bias, void* y, int64_t L, int64_t N, int64_t C, int K,
                                     int dt, js2t_stream stream) {
  if (L * N * C == 0) return JS2T_OK;
  JS2T_CHECK(x && w && y, "dwconv_outer_fwd: null pointer");
  JS2T_CHECK(K >= 1 && (K & 1) && K <= DW_MAXK, "dwconv_outer_fwd: kernel size must be odd and <= %d", DW_MAXK);
  if (dwconv_outer_win_launch<false>(x, w, bias, y, L, N, C, K, dt, (hipStream_t)stream) ||
      dwconv_outer_lds_launch<false>(x, w, bias, y, L, N, C, K, dt, (hipStream_t)stream)) {
    JS2T_LAUNCH_CHECK();
    return JS2T_OK;
  }
  DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_fwd_kernel<T>), dim3((unsigned)cdiv(L * N * C, 256)), dim3(256), 0,
                                        (hipStream_t)stream, (const T*)x, w, bias, (T*)y, L, N, C, K));
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

extern "C" int js2t_dwconv_outer_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, int64_t L, int64_t N, int64_t C,
                                     int K, int dt, js2t_stream stream) {
  if (L * N * C == 0) return JS2T_OK;
  JS2T_CHECK(dy && w, "dwconv_outer_bwd: null pointer");
  JS2T_CHECK(K >= 1 && (K & 1) && K <= DW_MAXK, "dwconv_outer_bwd: kernel size must be odd and <= %d", DW_MAXK);
  hipStream_t s = (hipStream_t)stream;
  if (dx && (dwconv_outer_win_launch<true>(dy, w, nullptr, dx, L, N, C, K, dt, s) || dwconv_outer_lds_launch<true>(dy, w, nullptr, dx, L, N, C, K, dt, s))) {
    JS2T_LAUNCH_CHECK();
  } else if (dx) {
    DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_dx_kernel<T>), dim3((unsigned)cdiv(L * N * C, 256)), dim3(256), 0, s,
                                          (const T*)dy, w, (T*)dx, L, N, C, K));
    JS2T_LAUNCH_CHECK();
  }
  if (dw) {
    JS2T_CHECK(x, "dwconv_outer_bwd: x needed for the weight gradient");
    JS2T_CHECK(cdiv(N, DW_SLAB) <= 65535, "dwconv_outer_bwd: too many rows");
    // columns per block: enough blocks for two per CU (the conv axis is the BATCH index, as in the reference: L is short, N long);
    // measured at L = 32, N = 375, C = 512: 4 -> 122 us, 8 -> 91, 16 -> 97, 32 -> 146 (dx + dw)
    int npb = (int)cdiv(N * cdiv(C, 64), 512);
    npb = npb < 4 ? 4 : (npb > DW_SLAB ? DW_SLAB : (npb + 3) & ~3);
    // the slabs' sums go through the library's scratch and are added up in order (also what deterministic mode wants); without the
    // scratch (first call under capture, or a problem larger than it): atomics, and in deterministic mode (js2t_set_deterministic)
    // ONE block per 64 channels that walks every column
    hipStreamCaptureStatus cap_state = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap_state);
    static bool scratch_ready = false;  // (the first, allocating call must be an eager one)
    float* part = nullptr;
    if (L < 65536 && N * C < (int64_t(1) << 30) && (scratch_ready || cap_state == hipStreamCaptureStatusNone)) {
      const char* e = getenv("JS2T_DW_NPB");
      const int npb_part = e ? atoi(e) : npb;
      part = dw_partial_scratch((size_t)cdiv(N, npb_part) * (size_t)C * (size_t)K);
      scratch_ready = true;
      if (part) npb = npb_part;
    }
    if (!part && g_js2t_deterministic && N < (1 << 30)) npb = (int)N;
    const dim3 grid((unsigned)cdiv(C, 64), (unsigned)cdiv(N, npb));
    if ((L >= 65536 || N * C >= (int64_t(1) << 30)) && !g_js2t_deterministic) {  // (int arithmetic of the window kernel)
      DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_dw_kernel<T>), dim3((unsigned)cdiv(C, 64), (unsigned)cdiv(N, DW_SLAB)), dim3(256),
                                            0, s, (const T*)dy, (const T*)x, dw, L, N, C, K));
    } else if (K <= 15) {
      DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_dw_win_kernel<T, 15, 32>), grid, dim3(256), 0, s, (const T*)dy, (const T*)x, dw,
                                            (int)L, N, C, K, npb, part));
    } else if (K <= 31) {
      DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_dw_win_kernel<T, 31, 16>), grid, dim3(256), 0, s, (const T*)dy, (const T*)x, dw,
                                            (int)L, N, C, K, npb, part));
    } else {
      DISPATCH_DT(dt, T, hipLaunchKernelGGL((dwconv_outer_dw_win_kernel<T, 63, 16>), grid, dim3(256), 0, s, (const T*)dy, (const T*)x, dw,
                                            (int)L, N, C, K, npb, part));
    }
    JS2T_LAUNCH_CHECK();
    if (part) {
      hipLaunchKernelGGL(dwconv_dw_reduce_kernel, dim3((unsigned)cdiv(C * K, 256)), dim3(256), 0, s, part, dw, C * (int64_t)K, (int)grid.y);
      JS2T_LAUNCH_CHECK();
    }
  }
  return JS2T_OK;
}

extern "C" int js2t_bn_act_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* mean,
                               float* invstd, void* y, float* ws, int64_t rows, int64_t C, float eps, float momentum, int train, int act,
                               int dt, js2t_stream stream) {
  if (rows * C == 0) return JS2T_OK;
  JS2T_CHECK(x && gamma && beta && mean && invstd && y, "bn_act_fwd: null pointer");
  JS2T_CHECK(train || (running_mean && running_var), "bn_act_fwd: eval mode needs running statistics");
  hipStream_t s = (hipStream_t)stream;
  const dim3 cgrid((unsigned)cdiv(C, 256));
  if (train) {
    JS2T_CHECK(ws, "bn_act_fwd: workspace required in train mode");
    JS2T_CHECK(cdiv(rows, BN_SLAB) <= 65535, "bn_act_fwd: too many rows");
    const int64_t slab = g_js2t_deterministic ? rows : BN_SLAB;  // deterministic mode: one block, one ordered sum per column
    const dim3 rgrid((unsigned)cdiv(C, 64), (unsigned)cdiv(rows, slab));
    hipError_t e = hipMemsetAsync(ws, 0, sizeof(float) * 2 * C, s);
    JS2T_CHECK(e == hipSuccess, "bn_act_fwd: memset failed: %s", hipGetErrorString(e));
    DISPATCH_DT(dt, T, hipLaunchKernelGGL((bn_colreduce_kernel<T, 0>), rgrid, dim3(256), 0, s, (const T*)x, (const T*)nullptr, nullptr,
                                          nullptr, nullptr, nullptr, ws, nullptr, rows, C, act, slab));
    JS2T_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_mean_kernel, cgrid, dim3(256), 0, s, ws, mean, rows, C);
    JS2T_LAUNCH_CHECK();
    DISPATCH_DT(dt, T, hipLaunchKernelGGL((bn_colreduce_kernel<T, 1>), rgrid, dim3(256), 0, s, (const T*)x, (const T*)nullptr, mean, nullptr,
                                          nullptr, nullptr, ws + C, nullptr, rows, C, act, slab));
    JS2T_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_finalize_kernel, cgrid, dim3(256), 0, s, ws + C, mean, invstd, running_mean, running_var, rows, C, eps,
                       momentum);
    JS2T_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(bn_eval_stats_kernel, cgrid, dim3(256), 0, s, running_mean, running_var, mean, invstd, C, eps);
    JS2T_LAUNCH_CHECK();
  }
  DISPATCH_DT(dt, T, hipLaunchKernelGGL((bn_act_apply_kernel<T>), dim3((unsigned)cdiv(rows * C, 256)), dim3(256), 0, s, (const T*)x, mean,
                                        invstd, gamma, beta, (T*)y, rows * C, C, act));
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

extern "C" int js2t_bn_act_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* invstd,
                               void* dx, float* dgamma, float* dbeta, float* ws, int64_t rows, int64_t C, int train, int act, int dt,
                               js2t_stream stream) {
  if (rows * C == 0) return JS2T_OK;
  JS2T_CHECK(dy && x && gamma && beta && mean && invstd && dx && ws, "bn_act_bwd: null pointer");
  JS2T_CHECK(cdiv(rows, BN_SLAB) <= 65535, "bn_act_bwd: too many rows");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws, 0, sizeof(float) * 2 * C, s);
  JS2T_CHECK(e == hipSuccess, "bn_act_bwd: memset failed: %s", hipGetErrorString(e));
  const int64_t slab = g_js2t_deterministic ? rows : BN_SLAB;
  const dim3 rgrid((unsigned)cdiv(C, 64), (unsigned)cdiv(rows, slab));
  DISPATCH_DT(dt, T, hipLaunchKernelGGL((bn_colreduce_kernel<T, 2>), rgrid, dim3(256), 0, s, (const T*)x, (const T*)dy, mean, invstd, gamma,
                                        beta, ws, ws + C, rows, C, act, slab));
  JS2T_LAUNCH_CHECK();
  DISPATCH_DT(dt, T, hipLaunchKernelGGL((bn_act_dx_kernel<T>), dim3((unsigned)cdiv(rows * C, 256)), dim3(256), 0, s, (const T*)dy,
                                        (const T*)x, mean, invstd, gamma, beta, ws, ws + C, (T*)dx, rows, C, act, train));
  JS2T_LAUNCH_CHECK();
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(bn_param_grad_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, s, ws, ws + C, dgamma, dbeta, C);
    JS2T_LAUNCH_CHECK();
  }
  return JS2T_OK;
}
