// The four-element output groups of the batch-assembly gathers (csrc/augment.hip, csrc/warp.hip): a thread holds four consecutive
// elements of an output row and stores them at once.
#pragma once
#include "common.h"

// elements 0 .. n - 1 of a group of four to p: one 16-byte store (4 bytes for 1-byte elements, two of 16 for 8-byte ones) when vec
template <typename T> __device__ __forceinline__ void store_group(T* __restrict__ p, const T (&v)[4], int n, int vec) {
    if (vec) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uchar4*>(p) = make_uchar4(v[0], v[1], v[2], v[3]);
        } else if constexpr (sizeof(T) == 4) {
            uint4 q;
            __builtin_memcpy(&q, v, 16);
            *reinterpret_cast<uint4*>(p) = q;
        } else {
            ulonglong2 q[2];
            __builtin_memcpy(q, v, 32);
            reinterpret_cast<ulonglong2*>(p)[0] = q[0];
            reinterpret_cast<ulonglong2*>(p)[1] = q[1];
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < n) p[t] = v[t];
    }
}

template <int BYTES> struct Elem;
template <> struct Elem<1> { typedef uint8_t type; };
template <> struct Elem<4> { typedef float type; };
template <> struct Elem<8> { typedef long long type; };
