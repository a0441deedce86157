// belief.h — the marginal belief of an acquisition's candidate as the kernels read it (BeliefArgs, dev.h): shared by ehvi.hip,
// cei.hip and mes.hip; nei.hip takes the clamp alone.
#pragma once
#include <cfloat>

#include "dev.h"

// The standard deviation of variance v: clamped as gp.hpp:621-623 — nothing at or below DBL_EPSILON is variance; a NaN stays one —
// then var_add (observation noise; 0: the latent function)
static __device__ __forceinline__ double belief_sigma(double v, double var_add)
{
    return sqrt((v > DBL_EPSILON ? v : (v != v ? v : 0.0)) + var_add);
}
// one model, several outputs: the sigma they share (b.var == null: not used, 0)
static __device__ __forceinline__ double belief_shared_sigma(const BeliefArgs& b, int64_t m)
{
    return b.var ? belief_sigma(b.var[m], b.var_add) : 0.0;
}
// the mean of belief j of candidate m
static __device__ __forceinline__ double belief_mean(const BeliefArgs& b, int64_t m, int j)
{
    double mu = b.mu[m + (int64_t)b.col[j] * b.ldmu];
    if (b.add)
        mu += b.add[m + (int64_t)j * b.lda];
    return mu;
}
// its standard deviation; sig: belief_shared_sigma of the candidate
static __device__ __forceinline__ double belief_sd(const BeliefArgs& b, int64_t m, int j, double sig)
{
    return b.var ? sig : b.sd[m + (int64_t)j * b.lds];
}
