// pk_lanes.h -- two 16-bit lanes in one 32-bit register, as the packed DP kernels hold two alignments per lane (band31_packed.hip,
// gotoh_full.hip): every add / max on a v2s is a v_pk_*_i16 doing two cells.
#pragma once
#include "common.h"

namespace nvbio_amd {

typedef short    v2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2s pk(const int a, const int b) { v2s r; r.x = (short)a; r.y = (short)b; return r; }
__device__ __forceinline__ v2s pk_max(const v2s a, const v2s b) { return __builtin_elementwise_max( a, b ); }
__device__ __forceinline__ v2s pk_bits(const uint32_t u) { return __builtin_bit_cast( v2s, u ); }
__device__ __forceinline__ uint32_t bits_pk(const v2s v) { return __builtin_bit_cast( uint32_t, v ); }
// the same pair of lanes as two binary16 numbers: every integer of magnitude <= 2048 is exact there, and gfx950 has a packed three-operand
// maximum (v_pk_maximum3_f16) where the integer pipe needs two v_pk_max_i16
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2h pk_max(const v2h a, const v2h b) { return __builtin_elementwise_maximum( a, b ); }
__device__ __forceinline__ v2s pk_max3(const v2s a, const v2s b, const v2s c) { return pk_max( pk_max( a, b ), c ); }
__device__ __forceinline__ v2h pk_max3(const v2h a, const v2h b, const v2h c) { return __builtin_elementwise_maximum( __builtin_elementwise_maximum( a, b ), c ); }
template <typename V> __device__ __forceinline__ V pk_of(const int a, const int b);
template <> __device__ __forceinline__ v2s pk_of<v2s>(const int a, const int b) { return pk( a, b ); }
template <> __device__ __forceinline__ v2h pk_of<v2h>(const int a, const int b) { v2h r; r.x = (_Float16)a; r.y = (_Float16)b; return r; }
template <bool FP> struct PkLanes { typedef v2s type; };
template <> struct PkLanes<true> { typedef v2h type; };

} // namespace nvbio_amd
