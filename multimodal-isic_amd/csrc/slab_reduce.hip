// The fixed-order slab reducers for a plain [slabs][n] stack (slab_sum.inc states the two orders): the second pass of the
// split-K GEMMs (gemm_f32.hip, gemm_f32t.hip), of the chunked column sums (gemm_f32.hip) and of the weight gradients whose
// slabs have the gradient's own layout (conv_wgrad.hip, conv_wgrad_c64.hip, conv_stem.hip).  Reducers with an epilogue of
// their own sit next to their producers and take only the sum from slab_sum.inc.
#include "slab_sum.inc"

#include "../../include/isic_hip_test.h"

namespace {

// Element i (four elements from i on) of a slab in the output.  MAP: rows of N elements lie ldc apart (the C of a GEMM);
// N == ldc is the contiguous output again.  The two forms that only the weight gradients use are built without the map.
template <bool MAP>
__device__ __forceinline__ float* slab_out(float* out, int64_t i, int N, int ldc) {
  return !MAP || N == ldc ? out + i : out + (i / N) * ldc + (i % N);
}

// order A: G lanes per element, 256 / G elements per block
template <int G, bool MAP>
__global__ __launch_bounds__(256) void slab_reduce_xor_kernel(const float* __restrict__ partial, int slabs, int64_t n,
                                                               float* __restrict__ out, int N, int ldc, float beta) {
  const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  const float s = isic_slab_sum_xor<G>(partial, (size_t)i, slabs, (size_t)n, i < n);
  if (i < n && threadIdx.x % G == 0) {
    float* p = slab_out<MAP>(out, i, N, ldc);
    *p = beta != 0.f ? beta * (*p) + s : s;
  }
}

// order B on f32x4: 16 x 4 elements per block.  The 16-lane form moves a 256 x 64 KB stack of partial GEMM tiles in 9.4 us,
// this one (every load of a thread independent, 16 in flight at 256 slabs) in half.
template <int ACC, bool MAP>
__global__ __launch_bounds__(256) void slab_reduce_lds16_kernel(const float* __restrict__ partial, int slabs, int64_t n,
                                                                 float* __restrict__ out, int N, int ldc, float beta) {
  const int64_t n4 = n / 4, e4 = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const f32x4 t = isic_slab_sum_lds16<ACC>(reinterpret_cast<const f32x4*>(partial), (size_t)e4, slabs, (size_t)n4, e4 < n4);
  if (threadIdx.x < 16 && e4 < n4) {
    f32x4* p = reinterpret_cast<f32x4*>(slab_out<MAP>(out, e4 * 4, N, ldc));
    *p = beta != 0.f ? beta * (*p) + t : t;
  }
}

// order B on scalars with four accumulators, as ct_slab_reduce_kernel (convmae_train.hip) forms it: test entry only
__global__ __launch_bounds__(256) void slab_reduce_lds16_s4_test_kernel(const float* __restrict__ partial, int slabs,
                                                                         int64_t n, float* __restrict__ out, float beta) {
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const float s = isic_slab_sum_lds16<4>(partial, (size_t)i, slabs, (size_t)n, i < n);
  if (threadIdx.x < 16 && i < n) out[i] = beta != 0.f ? beta * out[i] + s : s;
}

}  // namespace

// out[(i / N) * ldc + i % N] = beta * ... + sum; the forms without the map take N == ldc only
static void slab_reduce_launch(IsicSlabForm form, const float* partial, int slabs, int64_t n, float* out, int N, int ldc,
                               float beta, hipStream_t stream) {
  const int per_block = form == ISIC_SLAB_XOR16 ? 16 : 64;         // elements a block of 256 threads covers
  const auto kernel = form == ISIC_SLAB_XOR16 ? slab_reduce_xor_kernel<16, true>
                      : form == ISIC_SLAB_XOR4 ? slab_reduce_xor_kernel<4, false>
                      : form == ISIC_SLAB_LDS16_V1 ? slab_reduce_lds16_kernel<1, true> : slab_reduce_lds16_kernel<2, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(n, per_block)), dim3(256), 0, stream, partial, slabs, n, out, N, ldc, beta);
}

void isic_slab_reduce_launch(IsicSlabForm form, const float* partial, int slabs, int64_t n, float* out, float beta,
                             hipStream_t stream) {
  slab_reduce_launch(form, partial, slabs, n, out, 0, 0, beta, stream);
}

void isic_gemm_split_reduce_launch(const float* partial, int splits, float* C, int M, int N, int ldc, float beta,
                                   hipStream_t stream) {
  const bool vec = N % 4 == 0 && ldc % 4 == 0 && ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(C)) & 15) == 0;
  slab_reduce_launch(vec ? ISIC_SLAB_LDS16_V1 : ISIC_SLAB_XOR16, partial, splits, (int64_t)M * N, C, N, ldc, beta, stream);
}

extern "C" int isic_test_slab_reduce_f32(int form, const float* partial, int slabs, int64_t n, float* out, float beta,
                                         void* stream) {
  ISIC_CHECK_ARG(form >= 0 && form <= 4 && slabs >= 1 && n >= 0 && n <= (int64_t)0x7FFFFFFF * 16 && (beta == 0.f || beta == 1.f));
  if (n == 0) return ISIC_OK;
  ISIC_CHECK_ARG(partial && out);
  if (form == ISIC_SLAB_LDS16_V1 || form == ISIC_SLAB_LDS16_V2)
    ISIC_CHECK_ARG(n % 4 == 0 && ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(out)) & 15) == 0);
  if (form == 4)
    hipLaunchKernelGGL(slab_reduce_lds16_s4_test_kernel, dim3((unsigned)ceil_div64(n, 16)), dim3(256), 0, as_stream(stream),
                       partial, slabs, n, out, beta);
  else
    isic_slab_reduce_launch((IsicSlabForm)form, partial, slabs, n, out, beta, as_stream(stream));
  return isic_launch_status();
}
