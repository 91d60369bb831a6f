// The likelihood MLP of the factorized entropy bottleneck (reference entropy_model.py:82-101) as device routines, shared by the CDF-table
// kernels (entropy.hip) and the per-element likelihood kernel (loss.hip): both evaluate the same fp64 operation sequence.
// params packing (352 floats for C=8): matrices 0..3 [C,fo,fi] | biases 0..3 [C,fo,1] | factors 0..3 [C,fo,1], filters (1,3,3,3,1).
#pragma once
#include "pcgc_common.h"

__device__ static inline double eb_softplus(double x) { return x > 0 ? x + log1p(exp(-x)) : log1p(exp(x)); }
__device__ static inline double eb_sigmoid(double x) { return x >= 0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x)); }
// The parameter-only factors of the 4-layer chain — softplus(matrix) (24 per channel) and tanh(factor) (10 per channel) —
// are evaluated once per block into LDS; a table entry then costs 2 x 10 tanh + 2 sigmoid instead of 2 x 68 fp64
// transcendentals (the two table kernels sit on the critical path of encode and decode: 42 -> ~12 us each).  Same values,
// same operation order as evaluating them in place.
constexpr int EB_MAX_C = 16;
struct EbShared { double sp[EB_MAX_C * 24]; double tf[EB_MAX_C * 10]; };
__device__ static void eb_prepare(const float* __restrict__ P, int C, EbShared& sh) {
    const float* M = P; const float* Fa = P + 24 * C + 10 * C;
    const int F[5] = {1, 3, 3, 3, 1};
    for (int e = threadIdx.x; e < C * 34; e += blockDim.x) {
        const int c = e / 34, r = e % 34;
        if (r < 24) {                                   // matrix entry: local index -> (layer i, position inside the layer)
            int i = r < 3 ? 0 : (r < 12 ? 1 : (r < 21 ? 2 : 3));
            const int loff = i == 0 ? 0 : (i == 1 ? 3 : (i == 2 ? 12 : 21));
            int moff = 0;
            for (int j = 0; j < i; ++j) moff += C * F[j + 1] * F[j];
            sh.sp[c * 24 + r] = eb_softplus((double)M[moff + c * F[i + 1] * F[i] + (r - loff)]);
        } else {
            const int q = r - 24;                       // factor entry 0..9: layers of 3, 3, 3, 1
            const int i = q < 3 ? 0 : (q < 6 ? 1 : (q < 9 ? 2 : 3));
            const int boff = C * 3 * i;
            sh.tf[c * 10 + q] = tanh((double)Fa[boff + c * F[i + 1] + (q - 3 * i)]);
        }
    }
}
__device__ static double eb_logits(const float* __restrict__ P, int C, int c, double v, const EbShared& sh) {
    const int F[5] = {1, 3, 3, 3, 1};
    const float* B = P + 24 * C;
    const double* sp = sh.sp + c * 24; const double* tf = sh.tf + c * 10;
    double h[3] = {v, 0, 0}, t[3];
    int loff = 0, boff = 0, foff = 0;
    for (int i = 0; i < 4; ++i) {
        int fi = F[i], fo = F[i + 1];
        const float* b = B + boff + c * fo;
        for (int r = 0; r < fo; ++r) {
            double s = 0;
            for (int q = 0; q < fi; ++q) s += sp[loff + r * fi + q] * h[q];
            s += (double)b[r];
            s += tf[foff + r] * tanh(s);
            t[r] = s;
        }
        for (int r = 0; r < fo; ++r) h[r] = t[r];
        loff += fo * fi; boff += C * fo; foff += fo;
    }
    return h[0];
}
