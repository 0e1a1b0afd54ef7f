// What "this pixel is set" means for every kernel that reads masks (include/sola_hip.h, seg_utils._mask_kind), and how mask
// elements are read as bits.  The one statement of it on the device: the mask files include this and keep no copy.
//
// elem_type = element kind:
//   0  uint8    != 0
//   1  float32  != 0     (-0.0 clear, NaN SET)
//   2  float32  >  0     (tracker logits; -0.0 clear, NaN clear)
//   3  float32  <= 0     (the complement of 2 on numbers: -0.0 set, NaN clear)      sola_mask_components / _fill_small only
//   4  uint8    == 0                                                                 "
//   5  float32  == 0     (-0.0 set, NaN clear)                                       "
#pragma once
#include <type_traits>

#include "common.h"

constexpr int MASK_U8 = 0, MASK_F32 = 1, MASK_LOGIT = 2, MASK_LOGIT_CLEAR = 3, MASK_U8_CLEAR = 4, MASK_F32_CLEAR = 5;

template <int KIND>
struct mask_elem {
    using type = float;
    using vec = float4;  // 16 bytes of them, the unit of the vector reads
    static constexpr int size = 4;
};
template <>
struct mask_elem<MASK_U8> {
    using type = uint8_t;
    using vec = uint4;
    static constexpr int size = 1;
};
template <>
struct mask_elem<MASK_U8_CLEAR> : mask_elem<MASK_U8> {};

// thr: kind 2 against a threshold other than 0 (sola_mask_logit_stats); every other kind ignores it
template <int KIND>
__device__ __forceinline__ bool mask_is_set(typename mask_elem<KIND>::type v, float thr = 0.f) {
    static_assert(KIND >= MASK_U8 && KIND <= MASK_F32_CLEAR, "element kind");
    if constexpr (KIND == MASK_U8) return v != 0;
    else if constexpr (KIND == MASK_F32) return v != 0.f;
    else if constexpr (KIND == MASK_LOGIT) return v > thr;
    else if constexpr (KIND == MASK_LOGIT_CLEAR) return v <= 0.f;
    else if constexpr (KIND == MASK_U8_CLEAR) return v == 0;
    else return v == 0.f;
}

// bytes != 0 of one dword: bit 0 of every such byte (no carry leaves a byte: 0x7f + 0x7f < 0x100) ...
__device__ __forceinline__ uint32_t nz_byte_flags(uint32_t d) { return ((((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u) >> 7; }
// ... and gathered into 4 bits, byte i -> bit i: four uint8 pixels
__device__ __forceinline__ uint32_t nz_byte_bits(uint32_t d) {
    const uint32_t nz = nz_byte_flags(d);
    return (nz & 1u) | ((nz >> 7) & 2u) | ((nz >> 14) & 4u) | ((nz >> 21) & 8u);
}

// 16 bytes of a row -> 16 (uint8) or 4 (float32) bits, pixel i in bit i.  (Floats are loaded as floats: a compare on a
// dword reinterpreted in registers compiles to integer code.)
template <int KIND>
__device__ __forceinline__ uint32_t vec_bits(typename mask_elem<KIND>::vec v, float thr = 0.f) {
    static_assert(KIND != MASK_U8_CLEAR, "no kernel reads kind 4 by vectors");
    if constexpr (KIND == MASK_U8) {
        return nz_byte_bits(v.x) | nz_byte_bits(v.y) << 4 | nz_byte_bits(v.z) << 8 | nz_byte_bits(v.w) << 12;
    } else {
        return (uint32_t)mask_is_set<KIND>(v.x, thr) | (uint32_t)mask_is_set<KIND>(v.y, thr) << 1 | (uint32_t)mask_is_set<KIND>(v.z, thr) << 2 |
               (uint32_t)mask_is_set<KIND>(v.w, thr) << 3;
    }
}

// f(std::integral_constant<int, kind>) for kind = elem_type; the caller has checked 0 <= elem_type <= MAX_KIND
template <int MAX_KIND, typename F>
void with_mask_kind(int elem_type, F&& f) {
    if constexpr (MAX_KIND > 0) {
        if (elem_type < MAX_KIND) return with_mask_kind<MAX_KIND - 1>(elem_type, f);
    }
    f(std::integral_constant<int, MAX_KIND>());
}

// The first two checks of every check_sizes (rle_encode.hip, png_encode.hip)
inline int check_mask_sizes(const char* what, int elem_type, int n, int h, int w) {
    SOLA_ARG(n > 0 && h > 0 && w > 0, "%s: bad sizes n=%d h=%d w=%d", what, n, h, w);
    SOLA_ARG(elem_type >= 0 && elem_type <= 2, "%s: elem_type %d (0=u8, 1=f32, 2=f32 logits)", what, elem_type);
    return SOLA_OK;
}

// A piece [lo, hi) of the pixels of one map, read by 16-byte vectors of V pixels wherever the ADDRESS is 16-byte aligned:
// [v_lo, v_hi) is the part of it that is whole aligned vectors (n_vec of them); the n_edge < 2 V pixels in front of and behind
// them (the first n_head in front) are read one by one.  base_mod = (address of the array / element size) mod V, first = the
// map's first pixel in the whole array.
struct MaskPiece {
    int v_lo, v_hi, n_vec, n_head, n_edge;
};
template <int V>
__device__ __forceinline__ MaskPiece mask_piece(int base_mod, long long first, int lo, int hi) {
    const int mis_lo = (int)(((long long)base_mod + first % V + lo) % V);
    const int mis_hi = (int)(((long long)base_mod + first % V + hi) % V);
    MaskPiece p;
    p.v_lo = min(hi, lo + (V - mis_lo) % V);
    p.v_hi = max(p.v_lo, hi - mis_hi);
    p.n_vec = (p.v_hi - p.v_lo) / V;
    p.n_head = p.v_lo - lo;
    p.n_edge = p.n_head + (hi - p.v_hi);
    return p;
}
