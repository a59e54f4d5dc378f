// common.cuh — shared device helpers for the gfx950 (CDNA4 / MI355X) kernels.
// Wave = 64 lanes everywhere in this tree; MFMA fragments follow the gfx950
// v_mfma_f32_16x16x32_{bf16,f16} register maps:
//   A[m][k]: lane l holds m = l&15, k = (l>>4)*8 + j   (j = 0..7, 16 B)
//   B[k][n]: lane l holds n = l&15, k = (l>>4)*8 + j
//   D[m][n]: lane l holds n = l&15, m = (l>>4)*4 + r   (r = 0..3)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned short bf16_t;   // raw bfloat16 bits
typedef unsigned short f16_t;    // raw IEEE half bits

typedef __attribute__((ext_vector_type(8))) short  frag_ab;    // 8 x 16-bit MFMA A/B operand (4 VGPRs)
typedef __attribute__((ext_vector_type(8))) __bf16 frag_bf;    // same bits, bf16-typed for the builtin
typedef __attribute__((ext_vector_type(8))) _Float16 frag_h;   // f16-typed
typedef __attribute__((ext_vector_type(4))) float  f32x4;

#define VLO_DEV __device__ __forceinline__

VLO_DEV float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }

// round-to-nearest-even float -> bf16 (what torch's .to(bfloat16) does).  clang lowers these casts to
// gfx950's v_cvt_pk_bf16_f32 and — unlike inline asm — schedules the VALU->MFMA operand hazard itself.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
VLO_DEV unsigned pack2bf(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
VLO_DEV bf16_t f2bf(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
// value after a bf16 rounding point, kept in a float register
VLO_DEV float rbf(float f) { return (float)(__bf16)f; }

VLO_DEV float h2f(f16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
VLO_DEV f16_t f2h(float f) { return __builtin_bit_cast(f16_t, (_Float16)f); }

VLO_DEV f32x4 mfma_bf16(frag_ab a, frag_ab b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(frag_bf, a), __builtin_bit_cast(frag_bf, b), c, 0, 0, 0);
}
VLO_DEV f32x4 mfma_f16(frag_ab a, frag_ab b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(frag_h, a), __builtin_bit_cast(frag_h, b), c, 0, 0, 0);
}

// v_mfma_f32_16x16x128_f8f6f4 on OCP e4m3 bytes (cbsz = blgp = 0; zero scale operands select the UNSCALED instruction): a lane's operand is
// 32 bytes = row / column l & 15, 32 of the 128 k's.  Which 32 is the caller's business — a dot product does not care about the order of its
// terms as long as A and B agree — so the operand is given as the two 16-byte halves the callers already hold (D layout = the 16x16x32 forms').
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
VLO_DEV f32x4 mfma_fp8_k128(frag_ab a0, frag_ab a1, frag_ab b0, frag_ab b1, f32x4 c) {
    const i32x8_t A = __builtin_shufflevector(__builtin_bit_cast(i32x4_t, a0), __builtin_bit_cast(i32x4_t, a1), 0, 1, 2, 3, 4, 5, 6, 7);
    const i32x8_t B = __builtin_shufflevector(__builtin_bit_cast(i32x4_t, b0), __builtin_bit_cast(i32x4_t, b1), 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, c, 0, 0, 0, 0, 0, 0);
}

VLO_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
VLO_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// block-wide sum for blocks of up to 1024 threads; `sm` needs 16 floats
VLO_DEV float block_sum(float v, float *sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += sm[i];
    return t;
}
VLO_DEV float block_max(float v, float *sm) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    float t = -INFINITY;
    for (int i = 0; i < nw; ++i) t = fmaxf(t, sm[i]);
    return t;
}

// fp8 e4m3 (OCP, gfx950's native format) -> bf16, exact: every e4m3 value is a bf16 value, so the f32 the converter
// returns is truncated, not rounded.  One 16-byte register = the 8 + 8 weights of two consecutive MFMA fragments.
typedef __attribute__((ext_vector_type(2))) float f32x2_cv;
template <bool HI>
VLO_DEV unsigned fp8x2_to_bf16x2(unsigned src) {          // bytes 0,1 (HI = false) or 2,3 of src
    const f32x2_cv v = __builtin_amdgcn_cvt_pk_f32_fp8((int)src, HI);
    return (__float_as_uint(v[0]) >> 16) | (__float_as_uint(v[1]) & 0xffff0000u);
}
VLO_DEV void fp8x16_to_bf16(frag_ab raw, frag_ab &f0, frag_ab &f1) {
    const uint4 u = __builtin_bit_cast(uint4, raw);
    f0 = __builtin_bit_cast(frag_ab, make_uint4(fp8x2_to_bf16x2<false>(u.x), fp8x2_to_bf16x2<true>(u.x),
                                                  fp8x2_to_bf16x2<false>(u.y), fp8x2_to_bf16x2<true>(u.y)));
    f1 = __builtin_bit_cast(frag_ab, make_uint4(fp8x2_to_bf16x2<false>(u.z), fp8x2_to_bf16x2<true>(u.z),
                                                  fp8x2_to_bf16x2<false>(u.w), fp8x2_to_bf16x2<true>(u.w)));
}
// one fragment (8 e4m3 bytes) -> 8 bf16: the fp8 KV pool's K / V^T pieces (llm_ops.hip)
VLO_DEV frag_ab fp8x8_to_bf16(uint2 u) {
    return __builtin_bit_cast(frag_ab, make_uint4(fp8x2_to_bf16x2<false>(u.x), fp8x2_to_bf16x2<true>(u.x),
                                                  fp8x2_to_bf16x2<false>(u.y), fp8x2_to_bf16x2<true>(u.y)));
}
// four values -> four OCP e4m3 bytes (byte r = value r): e4m3_rne(clamp(x / s, -448, 448)), the clamp-then-v_cvt_pk_fp8_f32 rule of
// quantize_rows_fp8_kernel (prefill.hip).  The fp8 KV cache's quantiser (s = the layer's k_scale / v_scale).
VLO_DEV unsigned fp8x4_quant(float a, float b, float c, float d, float s) {
    a = fminf(fmaxf(a / s, -448.f), 448.f); b = fminf(fmaxf(b / s, -448.f), 448.f);
    c = fminf(fmaxf(c / s, -448.f), 448.f); d = fminf(fmaxf(d / s, -448.f), 448.f);
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, lo, true);
}
VLO_DEV float fp8_to_f32(unsigned byte) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)byte, false)[0]; }

// OCP MXFP4 (vlo_config.weight_dtype = 2) -> bf16, exact.  A code is e2m1 (sign bit 3, exponent bits 2:1, mantissa bit 0: +-{0, 0.5, 1, 1.5,
// 2, 3, 4, 6}), a block of 32 codes along K shares one e8m0 scale byte e8 (2^(e8 - 127), 2 <= e8 <= 254 checked at load): every product
// code * scale is a bf16 value.  One dword = the 8 codes of one lane of one MFMA fragment (k ascending from the low nibble).
// gfx950 converts two codes per VALU operation (v_cvt_scalef32_pk_bf16_fp4, scale = the float 2^(e8 - 127)); a compiler without the builtin
// takes the integer arm, which gives the same bits: exponent field e8 + e - 1 (e8 - 1 for the sub-normal code 0.5), mantissa bit 6 = the
// code's mantissa bit, infinity where the product passes bf16's largest binade (e8 >= 253 only).
#if defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4)
#define VLO_HAS_CVT_SCALE_FP4 1
#endif
#endif
VLO_DEV unsigned fp4_to_bf16_bits(unsigned c, unsigned e8) {       // integer arm: one code -> bf16 bits
    const unsigned e = (c >> 1) & 3u, m = c & 1u;
    const unsigned ex = e ? e8 + e - 1u : e8 - 1u;
    unsigned b = e ? ((ex << 7) | (m << 6)) : (m ? (ex << 7) : 0u);
    if (ex >= 255u && (e | m)) b = 0x7f80u;
    return b | ((c & 8u) << 12);
}
template <int B>
VLO_DEV unsigned fp4x2_to_bf16x2(unsigned src, unsigned e8) {      // byte B of src: low nibble -> low half
#ifdef VLO_HAS_CVT_SCALE_FP4
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(src, __uint_as_float(e8 << 23), B));
#else
    const unsigned by = (src >> (8 * B)) & 0xffu;
    return fp4_to_bf16_bits(by & 15u, e8) | (fp4_to_bf16_bits(by >> 4, e8) << 16);
#endif
}
VLO_DEV frag_ab fp4x8_to_bf16(unsigned codes, unsigned e8) {       // one fragment of a lane
    return __builtin_bit_cast(frag_ab, make_uint4(fp4x2_to_bf16x2<0>(codes, e8), fp4x2_to_bf16x2<1>(codes, e8),
                                                  fp4x2_to_bf16x2<2>(codes, e8), fp4x2_to_bf16x2<3>(codes, e8)));
}
// one 16-byte register of the mxfp4 image (gemv.hip) = four consecutive fragments; `sc` = their four scale bytes, fragment 0 in the low byte
VLO_DEV void fp4x32_to_bf16(frag_ab raw, unsigned sc, frag_ab &f0, frag_ab &f1, frag_ab &f2, frag_ab &f3) {
    const uint4 u = __builtin_bit_cast(uint4, raw);
    f0 = fp4x8_to_bf16(u.x, sc & 0xffu);
    f1 = fp4x8_to_bf16(u.y, (sc >> 8) & 0xffu);
    f2 = fp4x8_to_bf16(u.z, (sc >> 16) & 0xffu);
    f3 = fp4x8_to_bf16(u.w, sc >> 24);
}
