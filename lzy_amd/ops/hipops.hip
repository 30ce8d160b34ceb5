// lzy_amd data-plane kernels for gfx950 (MI355X, CDNA4).
//
// These replace the reference's serializer byte-stream hot path (reference:
// pylzy snapshot.put_data md5+S3 upload, api/v1/snapshot.py:141-160; slots
// chunk streams, lzy/slots transfers/SlotInputTransfer.java): on MI355X a
// tensor crossing a channel stays in HBM and the only per-byte work is
// (a) optional dtype cast ("cast on the wire") and (b) content checksum for
// the result cache / dedup.  Both are HBM-bandwidth-bound: kernels are
// vectorized 16 B/lane, grid-stride, grid capped so blocks span all 8 XCDs.
//
// Wave size 64; block 256 threads; no CUDA compatibility paths.
//
// Checksum design: position-salted splitmix64 mixing, combined with a
// commutative sum so any processing order yields the same digest; each
// lane streams 16 B per iteration.  A second entry point (lz_checksum_mfma)
// folds the per-block digests through an i8 MFMA (matrix universal hash) —
// the bulk pass is identical (memory-bound either way; MFMA makes the
// combine arithmetic free and is profiled with rocprof counters).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_fp8.h>

#include <cstdint>
#include <type_traits>

#define LZ_BLOCK 256
// Default grid cap: 4 workgroups per CU.  Swept on MI355X (profiles/
// kernel_sweep.md): 1024 beats 2048..16384 on every data-plane kernel —
// persistent grid-stride loops keep each XCD's L2 working set small and
// the HBM streams long; larger grids only add launch/tail overhead.
#define LZ_MAX_BLOCKS 1024  // 256 CUs x 4 blocks/CU (runtime-tunable)

static int g_max_blocks = LZ_MAX_BLOCKS;
extern "C" void lz_set_max_blocks(int b) { g_max_blocks = b > 0 ? b : LZ_MAX_BLOCKS; }

// ---------------------------------------------------------------------------
// dtype codes shared with python (lzy_amd/ops/__init__.py)
// ---------------------------------------------------------------------------
enum LzDtype : int {
    LZ_F32 = 0,
    LZ_F16 = 1,
    LZ_BF16 = 2,
    LZ_FP8_E4M3 = 3,
    LZ_FP8_E5M2 = 4,
    LZ_U8 = 5,
    LZ_I32 = 6,
    LZ_I64 = 7,
    LZ_F64 = 8,
};

// ---------------------------------------------------------------------------
// cast_copy: dst[i] = cast(src[i]) — fused pack + dtype cast.
// ---------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ float lz_to_float(T v);

template <> __device__ __forceinline__ float lz_to_float<float>(float v) { return v; }
template <> __device__ __forceinline__ float lz_to_float<__half>(__half v) { return __half2float(v); }
template <> __device__ __forceinline__ float lz_to_float<__hip_bfloat16>(__hip_bfloat16 v) { return __bfloat162float(v); }
template <> __device__ __forceinline__ float lz_to_float<__hip_fp8_e4m3>(__hip_fp8_e4m3 v) { return float(v); }
template <> __device__ __forceinline__ float lz_to_float<__hip_fp8_e5m2>(__hip_fp8_e5m2 v) { return float(v); }
template <> __device__ __forceinline__ float lz_to_float<uint8_t>(uint8_t v) { return (float)v; }
template <> __device__ __forceinline__ float lz_to_float<int32_t>(int32_t v) { return (float)v; }
template <> __device__ __forceinline__ float lz_to_float<int64_t>(int64_t v) { return (float)v; }
template <> __device__ __forceinline__ float lz_to_float<double>(double v) { return (float)v; }

template <typename T>
__device__ __forceinline__ T lz_from_float(float v);

template <> __device__ __forceinline__ float lz_from_float<float>(float v) { return v; }
template <> __device__ __forceinline__ __half lz_from_float<__half>(float v) { return __float2half(v); }
template <> __device__ __forceinline__ __hip_bfloat16 lz_from_float<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ __hip_fp8_e4m3 lz_from_float<__hip_fp8_e4m3>(float v) { return __hip_fp8_e4m3(v); }
template <> __device__ __forceinline__ __hip_fp8_e5m2 lz_from_float<__hip_fp8_e5m2>(float v) { return __hip_fp8_e5m2(v); }
template <> __device__ __forceinline__ uint8_t lz_from_float<uint8_t>(float v) { return (uint8_t)v; }
template <> __device__ __forceinline__ int32_t lz_from_float<int32_t>(float v) { return (int32_t)v; }
template <> __device__ __forceinline__ int64_t lz_from_float<int64_t>(float v) { return (int64_t)v; }
template <> __device__ __forceinline__ double lz_from_float<double>(float v) { return (double)v; }

// One element of cast_copy.  Pairs of plain arithmetic types (f32, f64, i32,
// i64, u8) convert directly, so i32/i64/f64 keep every bit the destination
// can hold; any pair with a 16- or 8-bit float goes through f32, the only
// conversion those types have (f64 -> bf16 is therefore double-rounded).
template <typename T>
inline constexpr bool lz_is_plain =
    std::is_same<T, float>::value || std::is_same<T, double>::value ||
    std::is_same<T, int32_t>::value || std::is_same<T, int64_t>::value ||
    std::is_same<T, uint8_t>::value;

template <typename SrcT, typename DstT>
__device__ __forceinline__ DstT lz_convert(SrcT v) {
    if constexpr (lz_is_plain<SrcT> && lz_is_plain<DstT>)
        return static_cast<DstT>(v);
    else
        return lz_from_float<DstT>(lz_to_float<SrcT>(v));
}

// Vectorized cast: each lane handles 8 contiguous elements per iteration
// (G13: hipcc does not auto-vectorize half-width loads; short4/short8
// reinterpret is the coalescing sweet spot).
template <typename SrcT, typename DstT>
__global__ void cast_copy_kernel(const SrcT* __restrict__ src,
                                 DstT* __restrict__ dst, int64_t n) {
    constexpr int V = 8;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t vec_n = n / V;

    using SrcV = struct { SrcT v[V]; };
    using DstV = struct { DstT v[V]; };
    const SrcV* srcv = reinterpret_cast<const SrcV*>(src);
    DstV* dstv = reinterpret_cast<DstV*>(dst);

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vec_n;
         i += stride) {
        SrcV s = srcv[i];
        DstV d;
#pragma unroll
        for (int k = 0; k < V; ++k) d.v[k] = lz_convert<SrcT, DstT>(s.v[k]);
        dstv[i] = d;
    }
    // tail
    int64_t tail_start = vec_n * V;
    for (int64_t i = tail_start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        dst[i] = lz_convert<SrcT, DstT>(src[i]);
    }
}

template <typename SrcT>
static hipError_t launch_cast_from(const void* src, void* dst, int dst_dtype,
                                   int64_t n, hipStream_t stream) {
    int64_t want = (n / 8 + LZ_BLOCK - 1) / LZ_BLOCK;
    int blocks = (int)(want < 1 ? 1 : (want > g_max_blocks ? g_max_blocks : want));
    switch (dst_dtype) {
#define LZ_CASE(code, T)                                                      \
    case code:                                                                \
        hipLaunchKernelGGL((cast_copy_kernel<SrcT, T>), dim3(blocks),         \
                           dim3(LZ_BLOCK), 0, stream, (const SrcT*)src,       \
                           (T*)dst, n);                                       \
        break;
        LZ_CASE(LZ_F32, float)
        LZ_CASE(LZ_F16, __half)
        LZ_CASE(LZ_BF16, __hip_bfloat16)
        LZ_CASE(LZ_FP8_E4M3, __hip_fp8_e4m3)
        LZ_CASE(LZ_FP8_E5M2, __hip_fp8_e5m2)
        LZ_CASE(LZ_U8, uint8_t)
        LZ_CASE(LZ_I32, int32_t)
        LZ_CASE(LZ_I64, int64_t)
        LZ_CASE(LZ_F64, double)
#undef LZ_CASE
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" hipError_t lz_cast_copy(const void* src, int src_dtype, void* dst,
                                   int dst_dtype, int64_t n, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    switch (src_dtype) {
        case LZ_F32: return launch_cast_from<float>(src, dst, dst_dtype, n, s);
        case LZ_F16: return launch_cast_from<__half>(src, dst, dst_dtype, n, s);
        case LZ_BF16: return launch_cast_from<__hip_bfloat16>(src, dst, dst_dtype, n, s);
        case LZ_FP8_E4M3: return launch_cast_from<__hip_fp8_e4m3>(src, dst, dst_dtype, n, s);
        case LZ_FP8_E5M2: return launch_cast_from<__hip_fp8_e5m2>(src, dst, dst_dtype, n, s);
        case LZ_U8: return launch_cast_from<uint8_t>(src, dst, dst_dtype, n, s);
        case LZ_I32: return launch_cast_from<int32_t>(src, dst, dst_dtype, n, s);
        case LZ_I64: return launch_cast_from<int64_t>(src, dst, dst_dtype, n, s);
        case LZ_F64: return launch_cast_from<double>(src, dst, dst_dtype, n, s);
        default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------
// mx8 pack/unpack: block-scaled FP8 wire format (OCP MXFP8, docs/mxwire.md).
//
// Every 32 elements share one power-of-two scale byte (E8M0); the payload
// is one OCP e4m3fn byte per element.  Wire buffer for n elements, with
// nblk = ceil(n/32): payload bytes [0, 32*nblk), then nblk scale bytes.
// This is also the operand layout of gfx950's block-scaled MFMA.
//
// Work item = 8 consecutive elements ("group"): the 4 lanes of an aligned
// quad own one block and a wave covers 16 blocks at a time.  The loop bound
// is wave-uniform (every lane of a wave takes the same trips), so the
// cross-lane steps always run with all 64 lanes; lanes past the end carry
// zeros and store nothing.  The pack is VALU-bound before it is HBM-bound
// (docs/performance.md), hence the packed converts and DPP moves.
//
// ALIGNED: src/dst allow 16 B (payload: 8 B) vector accesses.  Views that
// are only element-aligned take the same kernel with per-element accesses.
// ---------------------------------------------------------------------------

struct alignas(16) LzVec16 { uint32_t w[4]; };
struct alignas(8) LzVec8 { uint32_t w[2]; };

// scale byte of a block from the raw bits of its finite amax (>= 0):
// the smallest 2^(b-127) with amax / 2^(b-127) <= 448 = 1.75 * 2^8
__device__ __forceinline__ uint32_t lz_mx8_scale_byte(uint32_t amax_bits) {
    int e = (int)((amax_bits >> 23) & 0xffu);
    int b = e - 8 + ((amax_bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    return (uint32_t)(b < 0 ? 0 : b);
}

// x * 2^(127-b), clamped to the e4m3 finite range, NaN kept.  The multiply
// is exact (power of two) and finite values never exceed 448 by the choice
// of b, so the explicit clamp only ever moves +-Inf.  med3 drops NaN, the
// select puts it back.  Which NaN reaches the convert is not relied on (a
// negative NaN input has been seen to arrive with its sign): the one wire
// byte of NaN, 0x7f, is made in lz_mx8_encode4, on the converted bytes.
__device__ __forceinline__ float lz_mx8_scaled(float x, float mult) {
    const float v = x * mult;
    const float c = __builtin_amdgcn_fmed3f(v, -448.f, 448.f);
    return (v != v) ? __uint_as_float(0x7fc00000u) : c;
}

// 4 floats -> 4 e4m3 bytes (byte k = element k), RNE: v_cvt_pk_fp8_f32, the
// hardware convert behind __hip_fp8_e4m3 (OCP e4m3fn on gfx950), two
// elements per instruction, written straight into the half-words of a dword.
// A NaN can leave the convert as 0x7f or 0xff (a negative NaN input came
// out as 0xff); the wire is deterministic and has one NaN byte, 0x7f, so the
// sign bit of a NaN byte is cleared here.  A byte is NaN iff its low 7
// bits are all ones: only then does adding 1 to them carry into bit 7 (and
// never beyond the byte), which gives the sign bits to clear.
__device__ __forceinline__ uint32_t lz_mx8_encode4(const float* f, float mult) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(lz_mx8_scaled(f[0], mult),
                                            lz_mx8_scaled(f[1], mult), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(lz_mx8_scaled(f[2], mult),
                                        lz_mx8_scaled(f[3], mult), w, true);
    const uint32_t u = (uint32_t)w;
    const uint32_t nan_sign = ((u & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u;
    return u & ~nan_sign;
}

// a lane's 8 elements as fp32.  FULL: all 8 lie inside [0, n) and src + e0
// is 16 B-aligned (one or two 16 B loads); otherwise guarded, zeros past n.
template <typename T, bool FULL>
__device__ __forceinline__ void lz_mx8_load(const T* __restrict__ src, int64_t e0,
                                            int64_t n, float (&f)[8]) {
    constexpr int V = 8;
    T x[V];
    if (FULL) {
        LzVec16 q[sizeof(T) * V / 16];
        const LzVec16* p = reinterpret_cast<const LzVec16*>(src + e0);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(T) * V / 16); ++k) q[k] = p[k];
        __builtin_memcpy(x, q, sizeof(x));
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            x[k] = (e0 + k < n) ? src[e0 + k] : lz_from_float<T>(0.f);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = lz_to_float<T>(x[k]);
}

// DPP lane moves (VALU, no LDS round trip).  Must run with all 64 lanes on.
// quad_perm:[a,b,c,d] = a | b<<2 | c<<4 | d<<6: lane i of a quad reads lane sel[i]
#define LZ_DPP_QUAD_XOR1 0xB1  // [1,0,3,2]
#define LZ_DPP_QUAD_XOR2 0x4E  // [2,3,0,1]
#define LZ_DPP_ROW_SHL(k) (0x100 + (k))  // lane i reads lane i+k of its 16-lane row
template <int CTRL>
__device__ __forceinline__ uint32_t lz_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

// quantize and store one group (8 elements of lane `lane`, group g); every
// lane of the wave calls this together.  FULL: all 64 groups of the wave
// are inside the tensor, no guards.
template <bool ALIGNED, bool FULL>
__device__ __forceinline__ void lz_mx8_emit(const float (&f)[8], int64_t g, int lane,
                                            int64_t ngroups, int64_t nblk,
                                            uint8_t* __restrict__ dst,
                                            uint8_t* __restrict__ scales) {
    // amax over the finite elements on raw bits (integer order == float
    // order for |x|).  Biased by one exponent step: Inf/NaN (exponent 255)
    // carry into the sign bit and lose every signed max.
    int32_t tmax = 0x00800000;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int32_t t = (int32_t)((__float_as_uint(f[k]) & 0x7fffffffu) + 0x00800000u);
        tmax = t > tmax ? t : tmax;
    }
    uint32_t amax = (uint32_t)tmax - 0x00800000u;
    // quad reduce: the 4 lanes of a block
    uint32_t o = lz_dpp<LZ_DPP_QUAD_XOR1>(amax);
    amax = o > amax ? o : amax;
    o = lz_dpp<LZ_DPP_QUAD_XOR2>(amax);
    amax = o > amax ? o : amax;

    const uint32_t b = lz_mx8_scale_byte(amax);
    const float mult = __uint_as_float((254u - b) << 23);
    const uint32_t lo = lz_mx8_encode4(&f[0], mult);
    const uint32_t hi = lz_mx8_encode4(&f[4], mult);
    // gather the 4 scale bytes of each 16-lane row into its first lane, so
    // a wave's 16 scale bytes leave as 4 adjacent dword stores
    uint32_t sw = b;
    sw |= lz_dpp<LZ_DPP_ROW_SHL(4)>(b) << 8;
    sw |= lz_dpp<LZ_DPP_ROW_SHL(8)>(b) << 16;
    sw |= lz_dpp<LZ_DPP_ROW_SHL(12)>(b) << 24;

    if (FULL || g < ngroups) {
        const int64_t e0 = g * 8;
        if (ALIGNED) {
            LzVec8 pv;
            pv.w[0] = lo;
            pv.w[1] = hi;
            *reinterpret_cast<LzVec8*>(dst + e0) = pv;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dst[e0 + k] = (uint8_t)(lo >> (8 * k));
                dst[e0 + 4 + k] = (uint8_t)(hi >> (8 * k));
            }
        }
        if ((lane & 15) == 0) {
            const int64_t blk = g >> 2;  // multiple of 4
            if (ALIGNED && (FULL || blk + 4 <= nblk)) {
                *reinterpret_cast<uint32_t*>(scales + blk) = sw;
            } else {
                for (int k = 0; k < 4 && blk + k < nblk; ++k)
                    scales[blk + k] = (uint8_t)(sw >> (8 * k));
            }
        }
    }
}

template <typename T, bool ALIGNED>
__global__ void __launch_bounds__(LZ_BLOCK)
mx8_pack_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst, int64_t n) {
    const int64_t nblk = (n + 31) >> 5;
    const int64_t ngroups = nblk * 4;
    uint8_t* __restrict__ scales = dst + nblk * 32;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    // g0, the group of the wave's lane 0, and every branch on it are
    // wave-uniform: the cross-lane steps always run with all 64 lanes.
    // Two groups per trip: on the unguarded fast path both 16 B loads issue
    // before either is consumed.  The guarded path takes the tail and
    // element-aligned tensors.
    for (int64_t g0 = (int64_t)blockIdx.x * blockDim.x + wave * 64; g0 < ngroups;
         g0 += 2 * stride) {
        const int64_t ga = g0 + lane, gb = ga + stride;
        float fa[8], fb[8];
        if (ALIGNED && (g0 + stride + 64) * 8 <= n) {
            lz_mx8_load<T, true>(src, ga * 8, n, fa);
            lz_mx8_load<T, true>(src, gb * 8, n, fb);
            lz_mx8_emit<true, true>(fa, ga, lane, ngroups, nblk, dst, scales);
            lz_mx8_emit<true, true>(fb, gb, lane, ngroups, nblk, dst, scales);
        } else {
            const bool two = g0 + stride < ngroups;
            lz_mx8_load<T, false>(src, ga * 8, n, fa);
            lz_mx8_emit<ALIGNED, false>(fa, ga, lane, ngroups, nblk, dst, scales);
            if (two) {
                lz_mx8_load<T, false>(src, gb * 8, n, fb);
                lz_mx8_emit<ALIGNED, false>(fb, gb, lane, ngroups, nblk, dst, scales);
            }
        }
    }
}

// one group (8 elements) of the decode, in two steps so that a caller with
// several groups per lane can issue every load before the first store.
// Step 1: the group's payload words and its block's scale byte.
template <bool ALIGNED>
__device__ __forceinline__ void lz_mx8_dec_load(const uint8_t* __restrict__ src,
                                                const uint8_t* __restrict__ scales,
                                                int64_t g, uint32_t (&w)[2],
                                                uint32_t& b) {
    const int64_t e0 = g * 8;
    if (ALIGNED) {
        LzVec8 pv = *reinterpret_cast<const LzVec8*>(src + e0);
        w[0] = pv.w[0];
        w[1] = pv.w[1];
    } else {
        w[0] = w[1] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[0] |= (uint32_t)src[e0 + k] << (8 * k);
            w[1] |= (uint32_t)src[e0 + 4 + k] << (8 * k);
        }
    }
    b = scales[g >> 2];
}

// Step 2: dequantize and store the elements of the group that lie in [0, n).
//
// SIGNED_ZERO: for f16 the compiler folds the multiply and the convert into
// one v_fma_mixlo_f16 (q * mult + 0), and -0 + 0 is +0: a negative-zero
// payload byte, or a negative value that underflows f16, would come out
// +0.0 where the format says -0.0.  Decoded tensors are hashed as bytes
// (device_checksum), so every decoder puts the sign back: two integer
// operations per f16 element.
template <typename T, bool ALIGNED, bool SIGNED_ZERO>
__device__ __forceinline__ void lz_mx8_dec_store(const uint32_t (&w)[2], uint32_t b,
                                                 T* __restrict__ dst, int64_t g,
                                                 int64_t n) {
    constexpr int V = 8;
    const int64_t e0 = g * V;
    const float mult = __uint_as_float(b ? (b << 23) : 0x00400000u);
    T y[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        __hip_fp8_e4m3 q;
        q.__x = (__hip_fp8_storage_t)(w[k >> 2] >> (8 * (k & 3)));
        const float v = float(q) * mult;
        y[k] = lz_from_float<T>(v);
        if constexpr (SIGNED_ZERO && std::is_same<T, __half>::value)
            y[k] = __ushort_as_half((unsigned short)(
                (__half_as_ushort(y[k]) & 0x7fffu) |
                ((__float_as_uint(v) >> 16) & 0x8000u)));
    }
    if (ALIGNED && e0 + V <= n) {
        LzVec16 q[sizeof(T) * V / 16];
        __builtin_memcpy(q, y, sizeof(y));
        LzVec16* p = reinterpret_cast<LzVec16*>(dst + e0);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(T) * V / 16); ++k) p[k] = q[k];
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (e0 + k < n) dst[e0 + k] = y[k];
    }
}

template <typename T, bool ALIGNED>
__global__ void __launch_bounds__(LZ_BLOCK)
mx8_unpack_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, int64_t n) {
    const int64_t nblk = (n + 31) >> 5;
    const int64_t ngroups = nblk * 4;
    const uint8_t* __restrict__ scales = src + nblk * 32;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;

    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups;
         g += stride) {
        if (g * 8 >= n) continue;  // padded tail of the last block
        uint32_t w[2], b;
        lz_mx8_dec_load<ALIGNED>(src, scales, g, w, b);
        lz_mx8_dec_store<T, ALIGNED, true>(w, b, dst, g, n);
    }
}

static inline int lz_mx8_grid(int64_t n) {
    int64_t ngroups = ((n + 31) >> 5) * 4;
    int64_t want = (ngroups + LZ_BLOCK - 1) / LZ_BLOCK;
    return (int)(want < 1 ? 1 : (want > g_max_blocks ? g_max_blocks : want));
}

// src: n elements of src_dtype (f32/f16/bf16); dst_u8: 33*ceil(n/32) bytes
extern "C" hipError_t lz_mx8_pack(const void* src, int src_dtype, void* dst_u8,
                                  int64_t n, void* stream) {
    if (src_dtype != LZ_F32 && src_dtype != LZ_F16 && src_dtype != LZ_BF16)
        return hipErrorInvalidValue;
    if (n < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = lz_mx8_grid(n);
    const bool aligned = (((uintptr_t)src & 15) == 0) && (((uintptr_t)dst_u8 & 7) == 0);
#define LZ_MXP_CASE(code, T)                                                    \
    case code:                                                                  \
        if (aligned)                                                            \
            hipLaunchKernelGGL((mx8_pack_kernel<T, true>), dim3(blocks),        \
                               dim3(LZ_BLOCK), 0, s, (const T*)src,             \
                               (uint8_t*)dst_u8, n);                            \
        else                                                                    \
            hipLaunchKernelGGL((mx8_pack_kernel<T, false>), dim3(blocks),       \
                               dim3(LZ_BLOCK), 0, s, (const T*)src,             \
                               (uint8_t*)dst_u8, n);                            \
        break;
    switch (src_dtype) {
        LZ_MXP_CASE(LZ_F32, float)
        LZ_MXP_CASE(LZ_F16, __half)
        LZ_MXP_CASE(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_MXP_CASE
    return hipGetLastError();
}

// src_u8: 33*ceil(n/32) bytes; dst: n elements of dst_dtype (f32/f16/bf16)
extern "C" hipError_t lz_mx8_unpack(const void* src_u8, void* dst, int dst_dtype,
                                    int64_t n, void* stream) {
    if (dst_dtype != LZ_F32 && dst_dtype != LZ_F16 && dst_dtype != LZ_BF16)
        return hipErrorInvalidValue;
    if (n < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = lz_mx8_grid(n);
    const bool aligned = (((uintptr_t)src_u8 & 7) == 0) && (((uintptr_t)dst & 15) == 0);
#define LZ_MXU_CASE(code, T)                                                    \
    case code:                                                                  \
        if (aligned)                                                            \
            hipLaunchKernelGGL((mx8_unpack_kernel<T, true>), dim3(blocks),      \
                               dim3(LZ_BLOCK), 0, s, (const uint8_t*)src_u8,    \
                               (T*)dst, n);                                     \
        else                                                                    \
            hipLaunchKernelGGL((mx8_unpack_kernel<T, false>), dim3(blocks),     \
                               dim3(LZ_BLOCK), 0, s, (const uint8_t*)src_u8,    \
                               (T*)dst, n);                                     \
        break;
    switch (dst_dtype) {
        LZ_MXU_CASE(LZ_F32, float)
        LZ_MXU_CASE(LZ_F16, __half)
        LZ_MXU_CASE(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_MXU_CASE
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// checksum: 64-bit content hash of a device buffer.
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// Each lane: 2 x u64 (16 B) per grid-stride iteration; per-position salt
// makes the hash order-sensitive while the combine (wrapping +) stays
// commutative, so block/lane order doesn't matter.
__global__ void checksum_kernel(const uint8_t* __restrict__ data,
                                int64_t nbytes,
                                unsigned long long* __restrict__ out) {
    const uint64_t* words = reinterpret_cast<const uint64_t*>(data);
    int64_t nwords = nbytes >> 3;
    int64_t vec_n = nwords >> 1;  // pairs of u64

    uint64_t acc = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    using U64x2 = struct { uint64_t a, b; };
    const U64x2* w2 = reinterpret_cast<const U64x2*>(words);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vec_n;
         i += stride) {
        U64x2 w = w2[i];
        acc += splitmix64(w.a ^ splitmix64((uint64_t)(2 * i)));
        acc += splitmix64(w.b ^ splitmix64((uint64_t)(2 * i + 1)));
    }
    // odd trailing word + tail bytes: one thread
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (nwords & 1) {
            acc += splitmix64(words[nwords - 1] ^ splitmix64((uint64_t)(nwords - 1)));
        }
        int tail = (int)(nbytes & 7);
        if (tail) {
            uint64_t last = 0;
            const uint8_t* p = data + (nwords << 3);
            for (int k = 0; k < tail; ++k) last |= ((uint64_t)p[k]) << (8 * k);
            acc += splitmix64(last ^ splitmix64((uint64_t)nwords) ^ 0xA5A5A5A5ULL);
        }
        acc += splitmix64((uint64_t)nbytes ^ 0x1234567890ABCDEFULL);
    }

    // wave reduce (64 lanes), then one atomic per wave
    for (int off = 32; off > 0; off >>= 1)
        acc += (uint64_t)__shfl_down((long long)acc, off, 64);
    if ((threadIdx.x & 63) == 0)
        atomicAdd(out, (unsigned long long)acc);
}

extern "C" hipError_t lz_checksum(const void* data, int64_t nbytes,
                                  unsigned long long* out_device, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(out_device, 0, 8, s);
    if (err != hipSuccess) return err;
    int64_t want = (nbytes / 16 + LZ_BLOCK - 1) / LZ_BLOCK;
    int blocks = (int)(want < 1 ? 1 : (want > g_max_blocks ? g_max_blocks : want));
    hipLaunchKernelGGL(checksum_kernel, dim3(blocks), dim3(LZ_BLOCK), 0, s,
                       (const uint8_t*)data, nbytes, out_device);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// checksum_mfma: matrix-universal-hash digest on the MFMA units.
//
// The bulk pass is HBM-bound either way; routing the mixing arithmetic
// through the i8 matrix cores (v_mfma_i32_32x32x32_i8, ~4.4 PO/s) leaves
// the VALU nearly idle: per 1 KiB tile one MFMA replaces ~1.6k VALU mix
// ops, so the kernel runs at the memory ceiling with MfmaUtil carrying
// the compute (verified with rocprofv3 PMC, see profiles/).
//
// Scheme: D += A · (X_t ^ salt(t)) over Z_2^32, where X_t is the next
// 1 KiB of data as a 32x32 i8 tile (each lane holds 16 bytes = its B
// fragment, loaded as one coalesced dwordx4), A is a fixed dense
// pseudo-random i8 matrix (generated in-register from splitmix64), and
// salt(t) makes the hash position-sensitive while the i32 accumulation
// stays commutative across tiles.  Final fold: per-lane position-salted
// splitmix of the 16 accumulators, wave reduction, one atomic per wave.
// Any fixed lane->matrix-element mapping is a valid hash basis, so B
// fragments are simply lane-linear memory.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) int lz_i32x4;
typedef __attribute__((ext_vector_type(16))) int lz_i32x16;

__global__ void checksum_mfma_kernel(const uint8_t* __restrict__ data,
                                     int64_t nbytes,
                                     unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;

    // A operand: fixed dense pseudo-random bytes per lane (4 dwords)
    lz_i32x4 a_frag;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        a_frag[r] = (int)(uint32_t)(splitmix64(0x5EEDULL * 131 + lane * 4 + r) | 0x01010101u);

    lz_i32x16 acc = {0};

    const int64_t ntiles = nbytes >> 10;  // 1 KiB tiles
    const int64_t wave_id = (int64_t)blockIdx.x * waves_per_block + wave;
    const int64_t wave_stride = (int64_t)gridDim.x * waves_per_block;
    const lz_i32x4* tiles = reinterpret_cast<const lz_i32x4*>(data);

    // 4 tiles per iteration: the loads issue back-to-back (4 KiB of HBM
    // requests in flight per wave) before the dependent salt+MFMA chain —
    // the kernel is HBM-latency-bound otherwise.
    constexpr int U = 4;
    int64_t t = wave_id;
    for (; t + (U - 1) * wave_stride < ntiles; t += (int64_t)U * wave_stride) {
        lz_i32x4 b[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            b[u] = tiles[(t + u * wave_stride) * 64 + lane];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t s = splitmix64((uint64_t)(t + u * wave_stride));
#pragma unroll
            for (int r = 0; r < 4; ++r)
                b[u][r] ^= (int)(uint32_t)(s >> ((r * 13) & 31));
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_frag, b[u], acc, 0, 0, 0);
        }
    }
    for (; t < ntiles; t += wave_stride) {
        lz_i32x4 b_frag = tiles[t * 64 + lane];
        const uint64_t s = splitmix64((uint64_t)t);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            b_frag[r] ^= (int)(uint32_t)(s >> ((r * 13) & 31));
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_frag, b_frag, acc, 0, 0, 0);
    }

    // fold accumulators with position salts
    uint64_t h = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        h += splitmix64((uint32_t)acc[r] ^ splitmix64((uint64_t)(lane * 16 + r)));

    // tail (< 1 KiB) + length: one thread via the scalar mix
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint8_t* p = data + (ntiles << 10);
        int64_t rem = nbytes - (ntiles << 10);
        const uint64_t* words = reinterpret_cast<const uint64_t*>(p);
        int64_t nwords = rem >> 3;
        for (int64_t i = 0; i < nwords; ++i)
            h += splitmix64(words[i] ^ splitmix64((uint64_t)(ntiles * 128 + i)));
        int tb = (int)(rem & 7);
        if (tb) {
            uint64_t last = 0;
            const uint8_t* q = p + (nwords << 3);
            for (int k = 0; k < tb; ++k) last |= ((uint64_t)q[k]) << (8 * k);
            h += splitmix64(last ^ 0xA5A5A5A5ULL);
        }
        h += splitmix64((uint64_t)nbytes ^ 0x1234567890ABCDEFULL);
    }

    for (int off = 32; off > 0; off >>= 1)
        h += (uint64_t)__shfl_down((long long)h, off, 64);
    if (lane == 0)
        atomicAdd(out, (unsigned long long)h);
}

extern "C" hipError_t lz_checksum_mfma(const void* data, int64_t nbytes,
                                       unsigned long long* out_device,
                                       void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(out_device, 0, 8, s);
    if (err != hipSuccess) return err;
    int64_t tiles = nbytes >> 10;
    int64_t want = (tiles / 4 + LZ_BLOCK / 64 - 1) / (LZ_BLOCK / 64);
    int blocks = (int)(want < 1 ? 1 : (want > g_max_blocks ? g_max_blocks : want));
    hipLaunchKernelGGL(checksum_mfma_kernel, dim3(blocks), dim3(LZ_BLOCK), 0, s,
                       (const uint8_t*)data, nbytes, out_device);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fused elementwise/reduction ops — the "standard op" toolkit for workflow
// stages.  Rationale (MI355X performance rule: HBM traffic is the budget):
// an unfused torch chain like `(x.float() - x.mean()) / x.std()` moves
// ~14 GB per 1 GiB bf16 shard across 6 kernels; the fused pair below moves
// 3.2 GB in 2.  All kernels: vectorized 8 elems/lane, persistent grids,
// f32 lane accumulation folded to f64 per wave (one f64 atomic per wave).
// ---------------------------------------------------------------------------

__device__ __forceinline__ double lz_wave_reduce_f64(double v) {
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return v;
}

// sum of x and x^2 (or |x| with ABS=1) in one pass; out[0]+=sum, out[1]+=sumsq
//
// Non-temporal (evict-first) vector load: a 1 GiB reduction stream is
// 32x the combined L2, so marking lines no-reuse keeps the caches from
// churning on data that is read exactly once.  16 B granules — callers
// fall back to cached loads when the vector is not 16 B-aligned in size.
typedef int lz_v4i_t __attribute__((ext_vector_type(4)));

template <typename VecT>
__device__ __forceinline__ VecT lz_nt_load(const VecT* p) {
    VecT r;
    const lz_v4i_t* s = reinterpret_cast<const lz_v4i_t*>(p);
    lz_v4i_t* d = reinterpret_cast<lz_v4i_t*>(&r);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(VecT) / 16); ++k)
        d[k] = __builtin_nontemporal_load(s + k);
    return r;
}

// Load pipeline: U=4 independent vector loads per iteration (64 B/lane in
// flight) with separate accumulator pairs — a single accumulate chain
// leaves the reduction HBM-latency-bound (measured 2.8 TB/s; the
// streaming kernels hit 5.4+).
template <typename T, bool ABS,
          int V = (sizeof(T) == 2) ? 16 : 8, int U = 4, int NT = 0>
__global__ void stats_kernel(const T* __restrict__ src, int64_t n,
                             double* __restrict__ out) {
    // Default 32 B per lane per vector load regardless of dtype width:
    // 16-bit inputs at V=8 (16 B) leave the read stream request-starved.
    // V/U are template-swept (lz_stats_variant + benchmarks/kernel_sweep)
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t vec_n = n / V;
    using SrcV = struct { T v[V]; };
    const SrcV* srcv = reinterpret_cast<const SrcV*>(src);

    float s[U] = {0.f}, s2[U] = {0.f};
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (U - 1) * stride < vec_n; i += (int64_t)U * stride) {
        SrcV x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (NT != 0 && sizeof(SrcV) % 16 == 0)
                x[u] = lz_nt_load(&srcv[i + u * stride]);
            else
                x[u] = srcv[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float f = lz_to_float<T>(x[u].v[k]);
                s[u] += ABS ? fabsf(f) : f;
                s2[u] = fmaf(f, f, s2[u]);
            }
        }
    }
    for (; i < vec_n; i += stride) {
        SrcV x = srcv[i];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float f = lz_to_float<T>(x.v[k]);
            s[0] += ABS ? fabsf(f) : f;
            s2[0] = fmaf(f, f, s2[0]);
        }
    }
    int64_t tail_start = vec_n * V;
    for (int64_t j = tail_start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         j < n; j += stride) {
        float f = lz_to_float<T>(src[j]);
        s[0] += ABS ? fabsf(f) : f;
        s2[0] = fmaf(f, f, s2[0]);
    }
    double ds = 0, ds2 = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) { ds += (double)s[u]; ds2 += (double)s2[u]; }
    ds = lz_wave_reduce_f64(ds);
    ds2 = lz_wave_reduce_f64(ds2);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], ds);
        atomicAdd(&out[1], ds2);
    }
}

// dst = cast((src - mean) * rstd): stats read from the device buffer the
// stats kernel filled — no host round-trip between the two passes.
template <typename SrcT, typename DstT>
__global__ void normalize_apply_kernel(const SrcT* __restrict__ src,
                                       DstT* __restrict__ dst, int64_t n,
                                       const double* __restrict__ stats,
                                       float eps) {
    // mean/var/rstd in double, as mean_std() forms them on the host: in f32
    // the S2/n - mean^2 cancellation loses rstd once |mean| >> std.  Once
    // per thread; only the per-element arithmetic below runs in f32.
    const double mean_d = stats[0] / (double)n;
    const double var_d = stats[1] / (double)n - mean_d * mean_d;
    const float mean = (float)mean_d;
    const float rstd = (float)(1.0 / sqrt(fmax(var_d, 0.0) + (double)eps));

    constexpr int V = 8;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t vec_n = n / V;
    using SrcV = struct { SrcT v[V]; };
    using DstV = struct { DstT v[V]; };
    const SrcV* srcv = reinterpret_cast<const SrcV*>(src);
    DstV* dstv = reinterpret_cast<DstV*>(dst);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vec_n;
         i += stride) {
        SrcV x = srcv[i];
        DstV d;
#pragma unroll
        for (int k = 0; k < V; ++k)
            d.v[k] = lz_from_float<DstT>((lz_to_float<SrcT>(x.v[k]) - mean) * rstd);
        dstv[i] = d;
    }
    int64_t tail_start = vec_n * V;
    for (int64_t i = tail_start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride)
        dst[i] = lz_from_float<DstT>((lz_to_float<SrcT>(src[i]) - mean) * rstd);
}

// dst = cast(src * a + b) — fused affine (one FMA per element)
template <typename SrcT, typename DstT>
__global__ void scale_shift_kernel(const SrcT* __restrict__ src,
                                   DstT* __restrict__ dst, int64_t n,
                                   float a, float b) {
    constexpr int V = 8;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t vec_n = n / V;
    using SrcV = struct { SrcT v[V]; };
    using DstV = struct { DstT v[V]; };
    const SrcV* srcv = reinterpret_cast<const SrcV*>(src);
    DstV* dstv = reinterpret_cast<DstV*>(dst);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vec_n;
         i += stride) {
        SrcV x = srcv[i];
        DstV d;
#pragma unroll
        for (int k = 0; k < V; ++k)
            d.v[k] = lz_from_float<DstT>(fmaf(lz_to_float<SrcT>(x.v[k]), a, b));
        dstv[i] = d;
    }
    int64_t tail_start = vec_n * V;
    for (int64_t i = tail_start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride)
        dst[i] = lz_from_float<DstT>(fmaf(lz_to_float<SrcT>(src[i]), a, b));
}

// dst = cast(alpha*a + beta*b) — fused binary combine (tree-merge stages)
template <typename SrcT, typename DstT>
__global__ void axpby_kernel(const SrcT* __restrict__ a,
                             const SrcT* __restrict__ b,
                             DstT* __restrict__ dst, int64_t n, float alpha,
                             float beta) {
    constexpr int V = 8;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t vec_n = n / V;
    using SrcV = struct { SrcT v[V]; };
    using DstV = struct { DstT v[V]; };
    const SrcV* av = reinterpret_cast<const SrcV*>(a);
    const SrcV* bv = reinterpret_cast<const SrcV*>(b);
    DstV* dstv = reinterpret_cast<DstV*>(dst);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vec_n;
         i += stride) {
        SrcV x = av[i], y = bv[i];
        DstV d;
#pragma unroll
        for (int k = 0; k < V; ++k)
            d.v[k] = lz_from_float<DstT>(
                fmaf(lz_to_float<SrcT>(x.v[k]), alpha,
                     lz_to_float<SrcT>(y.v[k]) * beta));
        dstv[i] = d;
    }
    int64_t tail_start = vec_n * V;
    for (int64_t i = tail_start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride)
        dst[i] = lz_from_float<DstT>(
            fmaf(lz_to_float<SrcT>(a[i]), alpha, lz_to_float<SrcT>(b[i]) * beta));
}

static inline int lz_grid_for(int64_t work_items) {
    int64_t want = (work_items + LZ_BLOCK - 1) / LZ_BLOCK;
    return (int)(want < 1 ? 1 : (want > g_max_blocks ? g_max_blocks : want));
}

// out_device: double[2], zeroed here; out[0]=sum(|x| if abs else x), out[1]=sum(x^2)
extern "C" hipError_t lz_stats(const void* src, int dtype, int64_t n, int use_abs,
                               double* out_device, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(out_device, 0, 16, s);
    if (err != hipSuccess) return err;
    int blocks = lz_grid_for(n / 8);
#define LZ_STATS_CASE(code, T)                                                  \
    case code:                                                                  \
        if (use_abs)                                                            \
            hipLaunchKernelGGL((stats_kernel<T, true>), dim3(blocks),           \
                               dim3(LZ_BLOCK), 0, s, (const T*)src, n,          \
                               out_device);                                     \
        else                                                                    \
            hipLaunchKernelGGL((stats_kernel<T, false>), dim3(blocks),          \
                               dim3(LZ_BLOCK), 0, s, (const T*)src, n,          \
                               out_device);                                     \
        break;
    switch (dtype) {
        LZ_STATS_CASE(LZ_F32, float)
        LZ_STATS_CASE(LZ_F16, __half)
        LZ_STATS_CASE(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_STATS_CASE
    return hipGetLastError();
}

// sweep-only entry: V/U variants of the stats reduction (the one
// data-plane kernel measurably below the reduction ceiling — checksum
// streams at ~4.2-4.6 TB/s, stats at ~3.2).  Variants are compiled for
// the 16-bit path (bf16/f16); best found becomes the default above.
extern "C" hipError_t lz_stats_variant(const void* src, int dtype, int64_t n,
                                       int use_abs, double* out_device,
                                       void* stream, int variant) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(out_device, 0, 16, s);
    if (err != hipSuccess) return err;
    int blocks = lz_grid_for(n / 8);
#define LZ_SV_LAUNCH_NT(T, V, U, NT)                                            \
    do {                                                                        \
        if (use_abs)                                                            \
            hipLaunchKernelGGL((stats_kernel<T, true, V, U, NT>),               \
                               dim3(blocks), dim3(LZ_BLOCK), 0, s,              \
                               (const T*)src, n, out_device);                   \
        else                                                                    \
            hipLaunchKernelGGL((stats_kernel<T, false, V, U, NT>),              \
                               dim3(blocks), dim3(LZ_BLOCK), 0, s,              \
                               (const T*)src, n, out_device);                   \
    } while (0)
#define LZ_SV_LAUNCH(T, V, U) LZ_SV_LAUNCH_NT(T, V, U, 0)
#define LZ_SV_DTYPE(T)                                                          \
    switch (variant) {                                                          \
        case 0: LZ_SV_LAUNCH(T, 16, 4); break;                                  \
        case 1: LZ_SV_LAUNCH(T, 16, 8); break;                                  \
        case 2: LZ_SV_LAUNCH(T, 32, 2); break;                                  \
        case 3: LZ_SV_LAUNCH(T, 32, 4); break;                                  \
        case 4: LZ_SV_LAUNCH(T, 8, 8); break;                                   \
        case 5: LZ_SV_LAUNCH(T, 16, 2); break;                                  \
        case 6: LZ_SV_LAUNCH(T, 8, 4); break;                                   \
        case 7: LZ_SV_LAUNCH_NT(T, 16, 4, 1); break;                            \
        case 8: LZ_SV_LAUNCH_NT(T, 8, 8, 1); break;                             \
        case 9: LZ_SV_LAUNCH_NT(T, 16, 2, 1); break;                            \
        default: return hipErrorInvalidValue;                                   \
    }
    switch (dtype) {
        case LZ_F16: { LZ_SV_DTYPE(__half) break; }
        case LZ_BF16: { LZ_SV_DTYPE(__hip_bfloat16) break; }
        case LZ_F32: {
            switch (variant) {
                case 0: LZ_SV_LAUNCH(float, 8, 4); break;
                case 1: LZ_SV_LAUNCH(float, 8, 8); break;
                case 2: LZ_SV_LAUNCH(float, 16, 2); break;
                case 3: LZ_SV_LAUNCH(float, 16, 4); break;
                case 4: LZ_SV_LAUNCH(float, 4, 8); break;
                case 5: LZ_SV_LAUNCH(float, 8, 2); break;
                case 6: LZ_SV_LAUNCH(float, 4, 4); break;
                case 7: LZ_SV_LAUNCH_NT(float, 8, 4, 1); break;
                case 8: LZ_SV_LAUNCH_NT(float, 16, 4, 1); break;
                case 9: LZ_SV_LAUNCH_NT(float, 8, 2, 1); break;
                default: return hipErrorInvalidValue;
            }
            break;
        }
        default: return hipErrorInvalidValue;
    }
#undef LZ_SV_DTYPE
#undef LZ_SV_LAUNCH
#undef LZ_SV_LAUNCH_NT
    return hipGetLastError();
}

extern "C" hipError_t lz_normalize_apply(const void* src, int src_dtype,
                                         void* dst, int dst_dtype, int64_t n,
                                         const double* stats_device, float eps,
                                         void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int blocks = lz_grid_for(n / 8);
#define LZ_NA_DST(SrcT, code, DstT)                                             \
    case code:                                                                  \
        hipLaunchKernelGGL((normalize_apply_kernel<SrcT, DstT>), dim3(blocks),  \
                           dim3(LZ_BLOCK), 0, s, (const SrcT*)src, (DstT*)dst,  \
                           n, stats_device, eps);                               \
        break;
#define LZ_NA_SRC(scode, SrcT)                                                  \
    case scode:                                                                 \
        switch (dst_dtype) {                                                    \
            LZ_NA_DST(SrcT, LZ_F32, float)                                      \
            LZ_NA_DST(SrcT, LZ_F16, __half)                                     \
            LZ_NA_DST(SrcT, LZ_BF16, __hip_bfloat16)                            \
            default: return hipErrorInvalidValue;                               \
        }                                                                       \
        break;
    switch (src_dtype) {
        LZ_NA_SRC(LZ_F32, float)
        LZ_NA_SRC(LZ_F16, __half)
        LZ_NA_SRC(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_NA_SRC
#undef LZ_NA_DST
    return hipGetLastError();
}

extern "C" hipError_t lz_scale_shift(const void* src, int src_dtype, void* dst,
                                     int dst_dtype, int64_t n, float a, float b,
                                     void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int blocks = lz_grid_for(n / 8);
#define LZ_SS_DST(SrcT, code, DstT)                                             \
    case code:                                                                  \
        hipLaunchKernelGGL((scale_shift_kernel<SrcT, DstT>), dim3(blocks),      \
                           dim3(LZ_BLOCK), 0, s, (const SrcT*)src, (DstT*)dst,  \
                           n, a, b);                                            \
        break;
#define LZ_SS_SRC(scode, SrcT)                                                  \
    case scode:                                                                 \
        switch (dst_dtype) {                                                    \
            LZ_SS_DST(SrcT, LZ_F32, float)                                      \
            LZ_SS_DST(SrcT, LZ_F16, __half)                                     \
            LZ_SS_DST(SrcT, LZ_BF16, __hip_bfloat16)                            \
            default: return hipErrorInvalidValue;                               \
        }                                                                       \
        break;
    switch (src_dtype) {
        LZ_SS_SRC(LZ_F32, float)
        LZ_SS_SRC(LZ_F16, __half)
        LZ_SS_SRC(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_SS_SRC
#undef LZ_SS_DST
    return hipGetLastError();
}

extern "C" hipError_t lz_axpby(const void* a, const void* b, int src_dtype,
                               void* dst, int dst_dtype, int64_t n, float alpha,
                               float beta, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int blocks = lz_grid_for(n / 8);
#define LZ_AX_DST(SrcT, code, DstT)                                             \
    case code:                                                                  \
        hipLaunchKernelGGL((axpby_kernel<SrcT, DstT>), dim3(blocks),            \
                           dim3(LZ_BLOCK), 0, s, (const SrcT*)a,                \
                           (const SrcT*)b, (DstT*)dst, n, alpha, beta);         \
        break;
#define LZ_AX_SRC(scode, SrcT)                                                  \
    case scode:                                                                 \
        switch (dst_dtype) {                                                    \
            LZ_AX_DST(SrcT, LZ_F32, float)                                      \
            LZ_AX_DST(SrcT, LZ_F16, __half)                                     \
            LZ_AX_DST(SrcT, LZ_BF16, __hip_bfloat16)                            \
            default: return hipErrorInvalidValue;                               \
        }                                                                       \
        break;
    switch (src_dtype) {
        LZ_AX_SRC(LZ_F32, float)
        LZ_AX_SRC(LZ_F16, __half)
        LZ_AX_SRC(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_AX_SRC
#undef LZ_AX_DST
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// mx8_axpby: dst = cast(alpha*a + beta*decode(wire)) — the combine of a
// wire-cast merge-tree edge with the MXFP8 decode fused in (docs/mxwire.md).
//
// The received chunk never exists in the plan dtype: unpack-to-temporary
// followed by axpby moves ~9 B/element of bf16 through HBM, this kernel ~5
// (2 + 33/32 read, 2 written).  Per element, with x = float(q) * 2^(b-127)
// taken in fp32 (exact for every b, the subnormal multiplier of b == 0
// included): dst = round(fmaf(float(a), alpha, x * beta)) — axpby_kernel's
// operation order with b[i] replaced by x, x never rounded to 16 bits.
//
// Work item = 8 consecutive elements as in the sibling mx8 kernels; the 4
// lanes of a block read the same scale byte; nothing crosses lanes.  Two
// groups per grid-stride trip: on the unguarded path both payload loads and
// both loads of `a` issue before either is consumed.  `a` and `dst` may be
// the same pointer (a lane reads its 8 elements before it writes them, and
// no other lane touches them), so neither is __restrict__ here.
// ---------------------------------------------------------------------------

typedef float lz_f32x2 __attribute__((ext_vector_type(2)));

// 8 payload bytes (lo: elements 0-3, hi: 4-7) -> fp32 * mult.  v_cvt_pk_f32_fp8
// converts two bytes per instruction; its half selector is an immediate.
__device__ __forceinline__ void lz_mx8_decode8(uint32_t lo, uint32_t hi, float mult,
                                               float (&x)[8]) {
    lz_f32x2 p;
    p = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false);
    x[0] = p.x * mult; x[1] = p.y * mult;
    p = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    x[2] = p.x * mult; x[3] = p.y * mult;
    p = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false);
    x[4] = p.x * mult; x[5] = p.y * mult;
    p = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    x[6] = p.x * mult; x[7] = p.y * mult;
}

__device__ __forceinline__ float lz_mx8_mult(uint32_t b) {
    return __uint_as_float(b ? (b << 23) : 0x00400000u);
}

// combine and store one group.  FULL: all 8 elements lie inside [0, n) and
// dst + e0 is 16 B-aligned (one or two 16 B stores); otherwise guarded.
template <typename DstT, bool FULL>
__device__ __forceinline__ void lz_mx8_axpby_store(const float (&fa)[8], uint32_t lo,
                                                   uint32_t hi, uint32_t b, DstT* dst,
                                                   int64_t e0, int64_t n, float alpha,
                                                   float beta) {
    constexpr int V = 8;
    float x[V];
    lz_mx8_decode8(lo, hi, lz_mx8_mult(b), x);
    DstT y[V];
#pragma unroll
    for (int k = 0; k < V; ++k)
        y[k] = lz_from_float<DstT>(fmaf(fa[k], alpha, x[k] * beta));
    if (FULL) {
        LzVec16 q[sizeof(DstT) * V / 16];
        __builtin_memcpy(q, y, sizeof(y));
        LzVec16* p = reinterpret_cast<LzVec16*>(dst + e0);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(DstT) * V / 16); ++k) p[k] = q[k];
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (e0 + k < n) dst[e0 + k] = y[k];
    }
}

// one group on the guarded path (the tail, and element-aligned views)
template <typename SrcT, typename DstT, bool ALIGNED>
__device__ __forceinline__ void lz_mx8_axpby_one(const SrcT* a, const uint8_t* __restrict__ wire,
                                                 const uint8_t* __restrict__ scales,
                                                 DstT* dst, int64_t g, int64_t n,
                                                 float alpha, float beta) {
    const int64_t e0 = g * 8;
    if (e0 >= n) return;  // padded tail of the last block
    uint32_t lo = 0, hi = 0;
    if (ALIGNED) {
        // payload bytes of the padded tail exist: [0, 32*nblk)
        LzVec8 pv = *reinterpret_cast<const LzVec8*>(wire + e0);
        lo = pv.w[0];
        hi = pv.w[1];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)wire[e0 + k] << (8 * k);
            hi |= (uint32_t)wire[e0 + 4 + k] << (8 * k);
        }
    }
    const uint32_t b = scales[g >> 2];
    float fa[8];
    if (ALIGNED && e0 + 8 <= n) {
        lz_mx8_load<SrcT, true>(a, e0, n, fa);
        lz_mx8_axpby_store<DstT, true>(fa, lo, hi, b, dst, e0, n, alpha, beta);
    } else {
        lz_mx8_load<SrcT, false>(a, e0, n, fa);
        lz_mx8_axpby_store<DstT, false>(fa, lo, hi, b, dst, e0, n, alpha, beta);
    }
}

template <typename SrcT, typename DstT, bool ALIGNED>
__global__ void __launch_bounds__(LZ_BLOCK)
mx8_axpby_kernel(const SrcT* a, const uint8_t* __restrict__ wire, DstT* dst, int64_t n,
                 float alpha, float beta) {
    const int64_t nblk = (n + 31) >> 5;
    const int64_t ngroups = nblk * 4;
    const uint8_t* __restrict__ scales = wire + nblk * 32;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;

    for (int64_t ga = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ga < ngroups;
         ga += 2 * stride) {
        const int64_t gb = ga + stride;
        if (ALIGNED && (gb + 1) * 8 <= n) {  // ga < gb: both groups whole
            const LzVec8 pa = *reinterpret_cast<const LzVec8*>(wire + ga * 8);
            const LzVec8 pb = *reinterpret_cast<const LzVec8*>(wire + gb * 8);
            const uint32_t ba = scales[ga >> 2], bb = scales[gb >> 2];
            float fa[8], fb[8];
            lz_mx8_load<SrcT, true>(a, ga * 8, n, fa);
            lz_mx8_load<SrcT, true>(a, gb * 8, n, fb);
            lz_mx8_axpby_store<DstT, true>(fa, pa.w[0], pa.w[1], ba, dst, ga * 8, n,
                                           alpha, beta);
            lz_mx8_axpby_store<DstT, true>(fb, pb.w[0], pb.w[1], bb, dst, gb * 8, n,
                                           alpha, beta);
        } else {
            lz_mx8_axpby_one<SrcT, DstT, ALIGNED>(a, wire, scales, dst, ga, n, alpha, beta);
            if (gb < ngroups)
                lz_mx8_axpby_one<SrcT, DstT, ALIGNED>(a, wire, scales, dst, gb, n, alpha,
                                                      beta);
        }
    }
}

// a: n elements of a_dtype; wire_u8: 33*ceil(n/32) bytes; dst: n elements of
// dst_dtype (both f32/f16/bf16).  dst == a is allowed, partial overlap is not.
extern "C" hipError_t lz_mx8_axpby(const void* a, int a_dtype, const void* wire_u8,
                                   void* dst, int dst_dtype, int64_t n, float alpha,
                                   float beta, void* stream) {
    if (a_dtype != LZ_F32 && a_dtype != LZ_F16 && a_dtype != LZ_BF16)
        return hipErrorInvalidValue;
    if (dst_dtype != LZ_F32 && dst_dtype != LZ_F16 && dst_dtype != LZ_BF16)
        return hipErrorInvalidValue;
    if (n < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = lz_mx8_grid(n);
    const bool aligned = (((uintptr_t)a & 15) == 0) && (((uintptr_t)dst & 15) == 0) &&
                         (((uintptr_t)wire_u8 & 7) == 0);
#define LZ_MXA_DST(SrcT, code, DstT)                                            \
    case code:                                                                  \
        if (aligned)                                                            \
            hipLaunchKernelGGL((mx8_axpby_kernel<SrcT, DstT, true>),            \
                               dim3(blocks), dim3(LZ_BLOCK), 0, s,              \
                               (const SrcT*)a, (const uint8_t*)wire_u8,         \
                               (DstT*)dst, n, alpha, beta);                     \
        else                                                                    \
            hipLaunchKernelGGL((mx8_axpby_kernel<SrcT, DstT, false>),           \
                               dim3(blocks), dim3(LZ_BLOCK), 0, s,              \
                               (const SrcT*)a, (const uint8_t*)wire_u8,         \
                               (DstT*)dst, n, alpha, beta);                     \
        break;
#define LZ_MXA_SRC(scode, SrcT)                                                 \
    case scode:                                                                 \
        switch (dst_dtype) {                                                    \
            LZ_MXA_DST(SrcT, LZ_F32, float)                                     \
            LZ_MXA_DST(SrcT, LZ_F16, __half)                                    \
            LZ_MXA_DST(SrcT, LZ_BF16, __hip_bfloat16)                           \
            default: return hipErrorInvalidValue;                               \
        }                                                                       \
        break;
    switch (a_dtype) {
        LZ_MXA_SRC(LZ_F32, float)
        LZ_MXA_SRC(LZ_F16, __half)
        LZ_MXA_SRC(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_MXA_SRC
#undef LZ_MXA_DST
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// transpose_cast: dst[c][r] = cast(src[r][c]) — LDS-staged 64x64 tiles.
//
// The pack kernel for non-contiguous (transposed) tensors: a naive
// transpose strides HBM on one side (uncoalesced 2- or 4-byte accesses,
// ~1/8th bandwidth); staging tiles through LDS makes BOTH the load and
// the store coalesced.  Tile 64x64, block 256 threads (4 waves), +1
// element row padding so the transposed LDS reads spread across banks.
// 160 KB LDS/CU easily holds the f32 tile (16.25 KB) at high occupancy.
// ---------------------------------------------------------------------------

#define LZ_TT 64  // transpose tile edge

template <typename SrcT, typename DstT>
__global__ void transpose_cast_kernel(const SrcT* __restrict__ src,
                                      DstT* __restrict__ dst, int64_t rows,
                                      int64_t cols) {
    __shared__ float tile[LZ_TT][LZ_TT + 1];

    const int64_t tile_r = (int64_t)blockIdx.y * LZ_TT;
    const int64_t tile_c = (int64_t)blockIdx.x * LZ_TT;

    // load: each of 256 threads covers 16 elements, row-major coalesced
    const int tx = threadIdx.x & (LZ_TT - 1);        // 0..63 within a row
    const int ty = threadIdx.x >> 6;                 // 0..3
    for (int r = ty; r < LZ_TT; r += 4) {
        int64_t gr = tile_r + r;
        int64_t gc = tile_c + tx;
        if (gr < rows && gc < cols)
            tile[r][tx] = lz_to_float<SrcT>(src[gr * cols + gc]);
    }
    __syncthreads();

    // store: dst is (cols x rows); walk dst rows coalesced, read LDS
    // transposed (the +1 padding keeps those reads conflict-free)
    for (int c = ty; c < LZ_TT; c += 4) {
        int64_t gdr = tile_c + c;      // dst row = src col
        int64_t gdc = tile_r + tx;     // dst col = src row
        if (gdr < cols && gdc < rows)
            dst[gdr * rows + gdc] = lz_from_float<DstT>(tile[tx][c]);
    }
}

// v2: fully vectorized interior tiles — float4 HBM transactions on BOTH
// sides.  Each thread loads/stores 4 consecutive elements; the LDS tile
// keeps +1-row padding and the transposed reads gather 4 scalars from
// 4 consecutive padded rows (65-element stride => consecutive banks).
template <typename SrcT, typename DstT>
__global__ void transpose_cast_kernel_v4(const SrcT* __restrict__ src,
                                         DstT* __restrict__ dst, int64_t rows,
                                         int64_t cols) {
    __shared__ float tile[LZ_TT][LZ_TT + 1];

    const int64_t tile_r = (int64_t)blockIdx.y * LZ_TT;
    const int64_t tile_c = (int64_t)blockIdx.x * LZ_TT;

    const int tx = threadIdx.x & 15;   // 16 threads x 4 elems = 64 cols
    const int ty = threadIdx.x >> 4;   // 0..15 rows per pass
    using SrcV4 = struct { SrcT v[4]; };
    using DstV4 = struct { DstT v[4]; };

    for (int r = ty; r < LZ_TT; r += 16) {
        const int64_t gr = tile_r + r;
        const int64_t gc = tile_c + tx * 4;
        SrcV4 x = *reinterpret_cast<const SrcV4*>(&src[gr * cols + gc]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            tile[r][tx * 4 + k] = lz_to_float<SrcT>(x.v[k]);
    }
    __syncthreads();

    for (int c = ty; c < LZ_TT; c += 16) {
        const int64_t gdr = tile_c + c;       // dst row = src col
        const int64_t gdc = tile_r + tx * 4;  // dst col = src row
        DstV4 d;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            d.v[k] = lz_from_float<DstT>(tile[tx * 4 + k][c]);
        *reinterpret_cast<DstV4*>(&dst[gdr * rows + gdc]) = d;
    }
}

extern "C" hipError_t lz_transpose_cast(const void* src, int src_dtype,
                                        void* dst, int dst_dtype,
                                        int64_t rows, int64_t cols,
                                        void* stream) {
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((cols + LZ_TT - 1) / LZ_TT),
              (unsigned)((rows + LZ_TT - 1) / LZ_TT));
    // interior-only fast path: every tile full and 16B-aligned
    if ((rows % LZ_TT == 0) && (cols % LZ_TT == 0)) {
#define LZ_TCV_DST(SrcT, code, DstT)                                            \
    case code:                                                                  \
        hipLaunchKernelGGL((transpose_cast_kernel_v4<SrcT, DstT>), grid,        \
                           dim3(LZ_BLOCK), 0, s, (const SrcT*)src, (DstT*)dst,  \
                           rows, cols);                                         \
        break;
#define LZ_TCV_SRC(scode, SrcT)                                                 \
    case scode:                                                                 \
        switch (dst_dtype) {                                                    \
            LZ_TCV_DST(SrcT, LZ_F32, float)                                     \
            LZ_TCV_DST(SrcT, LZ_F16, __half)                                    \
            LZ_TCV_DST(SrcT, LZ_BF16, __hip_bfloat16)                           \
            default: return hipErrorInvalidValue;                               \
        }                                                                       \
        break;
        switch (src_dtype) {
            LZ_TCV_SRC(LZ_F32, float)
            LZ_TCV_SRC(LZ_F16, __half)
            LZ_TCV_SRC(LZ_BF16, __hip_bfloat16)
            default: return hipErrorInvalidValue;
        }
#undef LZ_TCV_SRC
#undef LZ_TCV_DST
        return hipGetLastError();
    }
#define LZ_TC_DST(SrcT, code, DstT)                                             \
    case code:                                                                  \
        hipLaunchKernelGGL((transpose_cast_kernel<SrcT, DstT>), grid,           \
                           dim3(LZ_BLOCK), 0, s, (const SrcT*)src, (DstT*)dst,  \
                           rows, cols);                                         \
        break;
#define LZ_TC_SRC(scode, SrcT)                                                  \
    case scode:                                                                 \
        switch (dst_dtype) {                                                    \
            LZ_TC_DST(SrcT, LZ_F32, float)                                      \
            LZ_TC_DST(SrcT, LZ_F16, __half)                                     \
            LZ_TC_DST(SrcT, LZ_BF16, __hip_bfloat16)                            \
            default: return hipErrorInvalidValue;                               \
        }                                                                       \
        break;
    switch (src_dtype) {
        LZ_TC_SRC(LZ_F32, float)
        LZ_TC_SRC(LZ_F16, __half)
        LZ_TC_SRC(LZ_BF16, __hip_bfloat16)
        default: return hipErrorInvalidValue;
    }
#undef LZ_TC_SRC
#undef LZ_TC_DST
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// segcopy: many (src, dst, nbytes) byte copies in ONE launch — the gather
// that packs a container's tensor leaves into one wire buffer, and the
// scatter that copies a received buffer into user tensors
// (channels/bundle.py, docs/bundles.md).
// ---------------------------------------------------------------------------
//
// Table (int64, device memory): src_addr[nseg], dst_addr[nseg], nbytes[nseg],
// tile_start[nseg + 1].  Segment s owns tiles [tile_start[s], tile_start[s+1])
// of LZ_SEG_TILE bytes each (the last one partial); zero-length segments own
// none.  A workgroup grid-strides over tiles; the tile index is a function of
// blockIdx alone, so the binary search over tile_start and the table reads
// are wave-uniform (scalar loads).
//
// Tile size: 16 KiB = 256 lanes x 16 B x 4.  Every lane issues its 4
// independent 16 B loads before the first store, and at the default grid cap
// 4 workgroups share a CU, i.e. 16 loads per lane slot and 64 KiB per CU in
// flight — above the >= 8 loads per lane / ~32 KiB per CU at which a
// streaming read stops being latency-bound on MI355X.  Measured with the
// table already on the device (benchmarks/bundle_probe.py, "kernel"): 1 GiB
// moves at 5.0 TB/s read+written as one segment and as 512 mixed ones alike,
// the rate of a plain copy of one buffer, so a larger tile has nothing left
// to buy (32 and 64 KiB builds measured the same) and would only coarsen the
// balance of small leaves: a state_dict is mostly biases and norms of a few
// KiB.
//
// Access width: LZ_SEG_TILE is a multiple of 16, so every tile of a segment
// has the alignment of the segment's own (src | dst).  Both 16 B-aligned ->
// 16 B vectors; otherwise the widest power of two dividing both addresses,
// down to single bytes.  The < width trailing bytes of a tile go bytewise.
// Nothing before src / past src + nbytes is read; nothing outside
// [dst, dst + nbytes) is written except, with zero_pad_align > 0, the zero
// fill of [dst + nbytes, align_up(dst + nbytes, zero_pad_align)) by the
// segment's last tile (the pack direction: every byte of the packed buffer
// is then defined, so buffers compare and hash equal).
#ifndef LZ_SEG_TILE
#define LZ_SEG_TILE 16384
#endif
static_assert(LZ_SEG_TILE % (LZ_BLOCK * 16) == 0, "tile = whole 16 B sweeps");

extern "C" int lz_segcopy_tile() { return LZ_SEG_TILE; }

// The table holds addresses as integers.  A pointer made from one is a
// generic ("flat") pointer unless it is given the global address space by
// hand, and flat accesses wait for the LDS counter as well as the memory
// one.  Clang's native vector types (unlike uint4, a class) load and store
// through address-space-qualified pointers.
#define LZ_GLOBAL __attribute__((address_space(1)))
typedef uint32_t lz_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lz_u32x2 __attribute__((ext_vector_type(2)));

template <typename V>
__device__ __forceinline__ void lz_seg_tile_copy(uint64_t sa, uint64_t da,
                                                 int len) {
    constexpr int U = LZ_SEG_TILE / (LZ_BLOCK * 16);  // loads in flight per lane
    constexpr int SWEEP = U * LZ_BLOCK;
    const int nv = len / (int)sizeof(V);
    const LZ_GLOBAL V* sv = (const LZ_GLOBAL V*)sa;
    LZ_GLOBAL V* dv = (LZ_GLOBAL V*)da;
    const int tid = (int)threadIdx.x;
    int base = 0;
    // whole sweeps: U independent loads issued back to back, then U stores
    for (; base + SWEEP <= nv; base += SWEEP) {
        V r[U];
#pragma unroll
        for (int k = 0; k < U; ++k) r[k] = sv[base + k * LZ_BLOCK + tid];
#pragma unroll
        for (int k = 0; k < U; ++k) dv[base + k * LZ_BLOCK + tid] = r[k];
    }
    // the partial sweep: loads stay unconditional (index clamped into the
    // tile, so nothing outside it is read) and only the stores are guarded
    // — a branch around each load would make every one of them wait
    if (base < nv) {
        V r[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = base + k * LZ_BLOCK + tid;
            r[k] = sv[i < nv ? i : nv - 1];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = base + k * LZ_BLOCK + tid;
            if (i < nv) dv[i] = r[k];
        }
    }
    // trailing len % sizeof(V) bytes (< 16 <= LZ_BLOCK): one byte per lane
    const int t = nv * (int)sizeof(V) + tid;
    if (t < len)
        ((LZ_GLOBAL uint8_t*)da)[t] = ((const LZ_GLOBAL uint8_t*)sa)[t];
}

__global__ void __launch_bounds__(LZ_BLOCK)
segcopy_kernel(const int64_t* __restrict__ table, int64_t nseg, int64_t ntiles,
               int zero_pad_align) {
    const int64_t* __restrict__ src_addr = table;
    const int64_t* __restrict__ dst_addr = table + nseg;
    const int64_t* __restrict__ seg_bytes = table + 2 * nseg;
    const int64_t* __restrict__ tile_start = table + 3 * nseg;

    int64_t lo = 0;  // a block's tiles ascend, so its segment index does too
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // largest s with tile_start[s] <= tile; invariant
        // tile_start[lo] <= tile < tile_start[hi] (tile_start[0] == 0,
        // tile_start[nseg] == ntiles), so empty segments are skipped.  A
        // tile still inside the previous segment needs no search.
        if (tile >= tile_start[lo + 1]) {
            int64_t hi = nseg;
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (tile_start[mid] <= tile) lo = mid; else hi = mid;
            }
        }
        const int64_t nb = seg_bytes[lo];
        const int64_t off = (tile - tile_start[lo]) * (int64_t)LZ_SEG_TILE;
        const int64_t rest = nb - off;
        if (rest <= 0) continue;  // malformed table: never index past a segment
        const int len = (int)(rest < LZ_SEG_TILE ? rest : LZ_SEG_TILE);
        const uint64_t sa = (uint64_t)src_addr[lo] + (uint64_t)off;
        const uint64_t da = (uint64_t)dst_addr[lo] + (uint64_t)off;
        const unsigned mis = (unsigned)((sa | da) & 15u);
        if (mis == 0) lz_seg_tile_copy<lz_u32x4>(sa, da, len);
        else if ((mis & 7u) == 0) lz_seg_tile_copy<lz_u32x2>(sa, da, len);
        else if ((mis & 3u) == 0) lz_seg_tile_copy<uint32_t>(sa, da, len);
        else if ((mis & 1u) == 0) lz_seg_tile_copy<uint16_t>(sa, da, len);
        else lz_seg_tile_copy<uint8_t>(sa, da, len);

        if (zero_pad_align > 0 && rest <= LZ_SEG_TILE) {  // segment's last tile
            const uint64_t end = (uint64_t)dst_addr[lo] + (uint64_t)nb;
            const uint64_t a = (uint64_t)zero_pad_align;
            const int pad = (int)((end + a - 1) / a * a - end);
            LZ_GLOBAL uint8_t* p = (LZ_GLOBAL uint8_t*)end;
            for (int i = (int)threadIdx.x; i < pad; i += LZ_BLOCK) p[i] = 0;
        }
    }
}

// No allocation, synchronisation or copy here: the caller owns the device
// table and has ordered its upload before this launch on ``stream``.
extern "C" hipError_t lz_segcopy(const void* table_dev, int64_t nseg,
                                 int64_t ntiles, int zero_pad_align,
                                 void* stream) {
    if (nseg < 0 || ntiles < 0 || zero_pad_align < 0) return hipErrorInvalidValue;
    if (nseg == 0 || ntiles == 0) return hipSuccess;
    if (table_dev == nullptr) return hipErrorInvalidValue;
    int blocks = (int)(ntiles > g_max_blocks ? g_max_blocks : ntiles);
    hipLaunchKernelGGL(segcopy_kernel, dim3(blocks), dim3(LZ_BLOCK), 0,
                       (hipStream_t)stream, (const int64_t*)table_dev, nseg,
                       ntiles, zero_pad_align);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// segcodec: segcopy whose segments may also be MXFP8-encoded or -decoded on
// the way — a tensor bundle whose large float leaves cross the wire
// block-scaled (bundle_wire_cast, docs/bundles.md) is packed by ONE launch
// and decoded into the exact bundle layout by ONE launch.
// ---------------------------------------------------------------------------
//
// Table (int64, device memory): src_addr[nseg], dst_addr[nseg], count[nseg],
// mode[nseg], tile_start[nseg + 1].
//   mode LZ_SC_RAW          copy `count` BYTES, tiles of LZ_SEG_TILE bytes
//                           (the body of segcopy_kernel);
//   mode LZ_SC_ENC + dtype  src: `count` ELEMENTS of f32/f16/bf16 (LzDtype
//                           0/1/2), dst: their mx8 buffer, 33*nblk bytes;
//   mode LZ_SC_DEC + dtype  src: an mx8 buffer, dst: `count` elements.
// A coded segment's tiles are LZ_SEGCODEC_ELEMS elements: tile t owns
// elements [t*E, min((t+1)*E, n)), payload bytes at seg + t*E and scale bytes
// at seg + 32*nblk + t*E/32.  E is a multiple of LZ_BLOCK*8, so a tile is a
// whole number of sweeps of the workgroup at one 8-element group per lane,
// the 4 lanes of a block are an aligned quad as in mx8_pack_kernel, and
// E/32 is a multiple of 64: the 4-byte scale stores of lz_mx8_emit stay
// aligned and never straddle tiles.  A wired segment is therefore the bytes
// lz_mx8_pack writes for the same leaf (same device functions, and a block's
// bytes depend on the block's elements alone).  The decode is the body of
// mx8_unpack_kernel (lz_mx8_dec_store, the sign of an f16 zero kept), so
// both are byte-identical to the torch codec.
//
// Segment, mode and alignment class are functions of blockIdx and the table
// only: wave-uniform.  Every wave of the workgroup walks its groups with a
// wave-uniform bound, so the DPP steps of lz_mx8_emit run with all 64 lanes
// on; the guards sit inside emit.  Fast path: the tile lies wholly inside
// the leaf, the leaf is 16 B-aligned and the mx8 side 8 B-aligned (segments
// of a packed buffer are 128 B-aligned, so only a misaligned source VIEW
// falls off it) — every load of the tile is issued before the first store.
// Anything else, and each segment's last tile, takes the guarded path.
//
// Nothing before or past a source is read.  Encode writes the whole mx8
// buffer, 0x00 for the padded payload of the last block; decode writes the
// n elements.  With zero_pad_align > 0 the segment's last tile zero-fills
// from the end of what it wrote to the next multiple, as segcopy does.
// Nothing else is written.  Zero-count segments own no tile.
#ifndef LZ_SEGCODEC_ELEMS
#define LZ_SEGCODEC_ELEMS 8192
#endif
static_assert(LZ_SEGCODEC_ELEMS % (LZ_BLOCK * 8) == 0, "tile = whole group sweeps");

#define LZ_SC_RAW 0
#define LZ_SC_ENC 1  // + LzDtype (f32/f16/bf16): 1, 2, 3
#define LZ_SC_DEC 4  // + LzDtype: 4, 5, 6

extern "C" int lz_segcodec_tile_elems() { return LZ_SEGCODEC_ELEMS; }

// zero [end, align_up(end, a)) — one workgroup
__device__ __forceinline__ void lz_seg_zero_pad(uint64_t end, int zero_pad_align) {
    const uint64_t a = (uint64_t)zero_pad_align;
    const int pad = (int)((end + a - 1) / a * a - end);
    LZ_GLOBAL uint8_t* p = (LZ_GLOBAL uint8_t*)end;
    for (int i = (int)threadIdx.x; i < pad; i += LZ_BLOCK) p[i] = 0;
}

// The table's addresses become global-address-space pointers first (see
// LZ_GLOBAL above); the generic pointers the mx8 device functions take are
// casts of those, which the compiler folds back once they are inlined.
template <typename T>
__device__ __forceinline__ void lz_segcodec_encode_tile(uint64_t sa, uint64_t da,
                                                        int64_t n, int64_t tix) {
    constexpr int U = LZ_SEGCODEC_ELEMS / (LZ_BLOCK * 8);  // groups per lane
    constexpr int64_t TG = LZ_SEGCODEC_ELEMS / 8;          // groups per tile
    const T* __restrict__ src = (const T*)(const LZ_GLOBAL T*)sa;
    uint8_t* __restrict__ dst = (uint8_t*)(LZ_GLOBAL uint8_t*)da;
    const int64_t nblk = (n + 31) >> 5;
    const int64_t ngroups = nblk * 4;
    uint8_t* __restrict__ scales = dst + nblk * 32;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t gtile = tix * TG;
    const bool src_al = (sa & 15u) == 0, dst_al = (da & 7u) == 0;

    if (src_al && dst_al && (gtile + TG) * 8 <= n) {
        float f[U][8];
#pragma unroll
        for (int k = 0; k < U; ++k)
            lz_mx8_load<T, true>(src, (gtile + k * LZ_BLOCK + wave * 64 + lane) * 8,
                                 n, f[k]);
#pragma unroll
        for (int k = 0; k < U; ++k)
            lz_mx8_emit<true, true>(f[k], gtile + k * LZ_BLOCK + wave * 64 + lane,
                                    lane, ngroups, nblk, dst, scales);
        return;
    }
    // g0, the group of the wave's lane 0, and the bound on it are
    // wave-uniform: emit's cross-lane steps see all 64 lanes
    for (int k = 0; k < U; ++k) {
        const int64_t g0 = gtile + k * LZ_BLOCK + wave * 64;
        if (g0 >= ngroups) break;
        const int64_t g = g0 + lane;
        float f[8];
        lz_mx8_load<T, false>(src, g * 8, n, f);
        if (dst_al) lz_mx8_emit<true, false>(f, g, lane, ngroups, nblk, dst, scales);
        else lz_mx8_emit<false, false>(f, g, lane, ngroups, nblk, dst, scales);
    }
}

template <typename T, bool ALIGNED>
__device__ __forceinline__ void lz_segcodec_decode_groups(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ scales,
    T* __restrict__ dst, int64_t n, int64_t gtile) {
    constexpr int U = LZ_SEGCODEC_ELEMS / (LZ_BLOCK * 8);
    uint32_t w[U][2], b[U];
    // a group past the end re-reads the segment's first group (inside the
    // source whenever the segment owns a tile) and stores nothing
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int64_t g = gtile + k * LZ_BLOCK + (int)threadIdx.x;
        lz_mx8_dec_load<ALIGNED>(src, scales, g * 8 < n ? g : 0, w[k], b[k]);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int64_t g = gtile + k * LZ_BLOCK + (int)threadIdx.x;
        if (g * 8 < n) lz_mx8_dec_store<T, ALIGNED, true>(w[k], b[k], dst, g, n);
    }
}

template <typename T>
__device__ __forceinline__ void lz_segcodec_decode_tile(uint64_t sa, uint64_t da,
                                                        int64_t n, int64_t tix) {
    const uint8_t* __restrict__ src = (const uint8_t*)(const LZ_GLOBAL uint8_t*)sa;
    T* __restrict__ dst = (T*)(LZ_GLOBAL T*)da;
    const int64_t nblk = (n + 31) >> 5;
    const uint8_t* __restrict__ scales = src + nblk * 32;
    const int64_t gtile = tix * (LZ_SEGCODEC_ELEMS / 8);
    if ((sa & 7u) == 0 && (da & 15u) == 0)
        lz_segcodec_decode_groups<T, true>(src, scales, dst, n, gtile);
    else
        lz_segcodec_decode_groups<T, false>(src, scales, dst, n, gtile);
}

__global__ void __launch_bounds__(LZ_BLOCK)
segcodec_kernel(const int64_t* __restrict__ table, int64_t nseg, int64_t ntiles,
                int zero_pad_align) {
    const int64_t* __restrict__ src_addr = table;
    const int64_t* __restrict__ dst_addr = table + nseg;
    const int64_t* __restrict__ seg_count = table + 2 * nseg;
    const int64_t* __restrict__ seg_mode = table + 3 * nseg;
    const int64_t* __restrict__ tile_start = table + 4 * nseg;

    int64_t lo = 0;  // a block's tiles ascend, so its segment index does too
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // the search of segcopy_kernel
        if (tile >= tile_start[lo + 1]) {
            int64_t hi = nseg;
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (tile_start[mid] <= tile) lo = mid; else hi = mid;
            }
        }
        const int64_t cnt = seg_count[lo];
        const int mode = (int)seg_mode[lo];
        const int64_t tix = tile - tile_start[lo];
        const uint64_t sbase = (uint64_t)src_addr[lo];
        const uint64_t dbase = (uint64_t)dst_addr[lo];

        if (mode == LZ_SC_RAW) {
            const int64_t off = tix * (int64_t)LZ_SEG_TILE;
            const int64_t rest = cnt - off;
            if (rest <= 0) continue;  // malformed table: never index past a segment
            const int len = (int)(rest < LZ_SEG_TILE ? rest : LZ_SEG_TILE);
            const uint64_t sa = sbase + (uint64_t)off;
            const uint64_t da = dbase + (uint64_t)off;
            const unsigned mis = (unsigned)((sa | da) & 15u);
            if (mis == 0) lz_seg_tile_copy<lz_u32x4>(sa, da, len);
            else if ((mis & 7u) == 0) lz_seg_tile_copy<lz_u32x2>(sa, da, len);
            else if ((mis & 3u) == 0) lz_seg_tile_copy<uint32_t>(sa, da, len);
            else if ((mis & 1u) == 0) lz_seg_tile_copy<uint16_t>(sa, da, len);
            else lz_seg_tile_copy<uint8_t>(sa, da, len);
            if (zero_pad_align > 0 && rest <= LZ_SEG_TILE)  // segment's last tile
                lz_seg_zero_pad(dbase + (uint64_t)cnt, zero_pad_align);
            continue;
        }
        const int64_t rest = cnt - tix * (int64_t)LZ_SEGCODEC_ELEMS;
        if (rest <= 0) continue;  // malformed table
        const bool last = rest <= LZ_SEGCODEC_ELEMS;
        const int64_t nblk = (cnt + 31) >> 5;
        switch (mode) {
            case LZ_SC_ENC + LZ_F32: lz_segcodec_encode_tile<float>(sbase, dbase, cnt, tix); break;
            case LZ_SC_ENC + LZ_F16: lz_segcodec_encode_tile<__half>(sbase, dbase, cnt, tix); break;
            case LZ_SC_ENC + LZ_BF16: lz_segcodec_encode_tile<__hip_bfloat16>(sbase, dbase, cnt, tix); break;
            case LZ_SC_DEC + LZ_F32: lz_segcodec_decode_tile<float>(sbase, dbase, cnt, tix); break;
            case LZ_SC_DEC + LZ_F16: lz_segcodec_decode_tile<__half>(sbase, dbase, cnt, tix); break;
            case LZ_SC_DEC + LZ_BF16: lz_segcodec_decode_tile<__hip_bfloat16>(sbase, dbase, cnt, tix); break;
            default: continue;  // malformed table: touch nothing
        }
        if (zero_pad_align > 0 && last) {
            const int64_t wrote = mode < LZ_SC_DEC ? 33 * nblk
                : cnt * (mode == LZ_SC_DEC + LZ_F32 ? 4 : 2);
            lz_seg_zero_pad(dbase + (uint64_t)wrote, zero_pad_align);
        }
    }
}

// As lz_segcopy: the caller owns the device table and has ordered its upload
// before this launch on ``stream``.
extern "C" hipError_t lz_segcodec(const void* table_dev, int64_t nseg,
                                  int64_t ntiles, int zero_pad_align,
                                  void* stream) {
    if (nseg < 0 || ntiles < 0 || zero_pad_align < 0) return hipErrorInvalidValue;
    if (nseg == 0 || ntiles == 0) return hipSuccess;
    if (table_dev == nullptr) return hipErrorInvalidValue;
    int blocks = (int)(ntiles > g_max_blocks ? g_max_blocks : ntiles);
    hipLaunchKernelGGL(segcodec_kernel, dim3(blocks), dim3(LZ_BLOCK), 0,
                       (hipStream_t)stream, (const int64_t*)table_dev, nseg,
                       ntiles, zero_pad_align);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// fill_pattern: test/verification helper (deterministic device-side fill).
// ---------------------------------------------------------------------------

// mask!=0: each 16-bit lane is ANDed with it after mixing — e.g. 0x3FFF
// clamps bf16 exponents so the pattern is finite positive synthetic data
// (fused here: a separate torch bitwise_and_ pass costs 2x the buffer in
// HBM traffic — measured 389 us per 1 GiB shard, profiles/
// kernel_stats_bench_fused.md).
__global__ void fill_pattern_kernel(uint8_t* __restrict__ bytes, int64_t nbytes,
                                    uint64_t seed, uint64_t mask16) {
    uint64_t* __restrict__ data = reinterpret_cast<uint64_t*>(bytes);
    const int64_t nwords = nbytes >> 3;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t m = mask16 ? (mask16 * 0x0001000100010001ULL) : ~0ULL;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
         i += stride) {
        data[i] = splitmix64(seed ^ (uint64_t)i) & m;
    }
    // trailing nbytes % 8 bytes: the low bytes of word `nwords`, one thread
    const int tail = (int)(nbytes & 7);
    if (tail && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t w = splitmix64(seed ^ (uint64_t)nwords) & m;
        uint8_t* p = bytes + (nwords << 3);
        for (int k = 0; k < tail; ++k) p[k] = (uint8_t)(w >> (8 * k));
    }
}

static hipError_t lz_fill_launch(void* data, int64_t nbytes, uint64_t seed,
                                 uint64_t mask16, void* stream) {
    if (nbytes < 0) return hipErrorInvalidValue;
    if (nbytes == 0) return hipSuccess;
    int64_t nwords = nbytes >> 3;
    int64_t want = (nwords + LZ_BLOCK - 1) / LZ_BLOCK;
    int blocks = (int)(want < 1 ? 1 : (want > g_max_blocks ? g_max_blocks : want));
    hipLaunchKernelGGL(fill_pattern_kernel, dim3(blocks), dim3(LZ_BLOCK), 0,
                       (hipStream_t)stream, (uint8_t*)data, nbytes, seed, mask16);
    return hipGetLastError();
}

extern "C" hipError_t lz_fill_pattern(void* data, int64_t nbytes, uint64_t seed,
                                      void* stream) {
    return lz_fill_launch(data, nbytes, seed, 0ULL, stream);
}

extern "C" hipError_t lz_fill_pattern_masked(void* data, int64_t nbytes,
                                             uint64_t seed, uint64_t mask16,
                                             void* stream) {
    return lz_fill_launch(data, nbytes, seed, mask16 & 0xFFFFULL, stream);
}

extern "C" const char* lz_error_name(hipError_t err) { return hipGetErrorName(err); }
