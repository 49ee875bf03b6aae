// tpg_weno_face.hpp -- the fifth-order WENO face value, the ONE definition in the tree: R(q0..q4) of include/tripolar_hip_weno.h
// (k_weno_tracer_advection, tpg_weno_tracer_kernel.hpp) and W5(q0..q4) of include/tripolar_hip_weno_momentum.h (k_weno_momentum_advection,
// tpg_weno_momentum.hip), operation for operation, in the field type T with no contraction.  Beside it weno_face3, R3(q0..q2) of
// include/tripolar_hip_weno_xyz.h, and the order table of that header's z-faces (the ZW form of that kernel, tpg_weno_xyz.hip).
// [recalled: uniform-grid coefficients, Jiang-Shu smoothness indicators, WENO-Z weights, eps = 1e-8; parity unpinned, like every operator here]
#pragma once

namespace {

// |x|: a sign clear
__device__ __forceinline__ float abs_of(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double abs_of(double x) { return __builtin_fabs(x); }

// R(q0, q1, q2, q3, q4) of the rule: q2 is the upwind cell, q3 the downwind one
template <typename T>
__device__ __forceinline__ T weno_face(T q0, T q1, T q2, T q3, T q4)
{
    constexpr T K13 = T(1) / T(3), K76 = T(7) / T(6), K116 = T(11) / T(6), K56 = T(5) / T(6), K16 = T(1) / T(6);
    constexpr T K1312 = T(13) / T(12), K310 = T(3) / T(10), K35 = T(3) / T(5), K110 = T(1) / T(10);
    constexpr T EPS = T(1e-8);
    const T p2 = (K13 * q0 - K76 * q1) + K116 * q2;
    const T p1 = (K56 * q2 - K16 * q1) + K13 * q3;
    const T p0 = (K13 * q2 + K56 * q3) - K16 * q4;
    const T s2 = (q0 - T(2) * q1) + q2, d2 = (q0 - T(4) * q1) + T(3) * q2;
    const T s1 = (q1 - T(2) * q2) + q3, d1 = q1 - q3;
    const T s0 = (q2 - T(2) * q3) + q4, d0 = (T(3) * q2 - T(4) * q3) + q4;
    const T b2 = K1312 * (s2 * s2) + T(0.25) * (d2 * d2);
    const T b1 = K1312 * (s1 * s1) + T(0.25) * (d1 * d1);
    const T b0 = K1312 * (s0 * s0) + T(0.25) * (d0 * d0);
    const T tau = abs_of(b0 - b2);
    const T r0 = tau / (b0 + EPS), r1 = tau / (b1 + EPS), r2 = tau / (b2 + EPS);
    const T a0 = K310 * (T(1) + r0 * r0), a1 = K35 * (T(1) + r1 * r1), a2 = K110 * (T(1) + r2 * r2);
    return ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2);
}

// W5F(q0..q4; t0..t4) of include/tripolar_hip_weno_vi.h (k_weno_vi_finish, tpg_weno_vi.hip), the ONE definition: R above with the smoothness
// indicators b2, b1, b0 formed from t0..t4 and the candidates p2, p1, p0 from q0..q4 (Oceananigans' FunctionStencil).  W5F(q; q) is R(q),
// operation for operation
template <typename T>
__device__ __forceinline__ T weno_face_fs(T q0, T q1, T q2, T q3, T q4, T t0, T t1, T t2, T t3, T t4)
{
    constexpr T K13 = T(1) / T(3), K76 = T(7) / T(6), K116 = T(11) / T(6), K56 = T(5) / T(6), K16 = T(1) / T(6);
    constexpr T K1312 = T(13) / T(12), K310 = T(3) / T(10), K35 = T(3) / T(5), K110 = T(1) / T(10);
    constexpr T EPS = T(1e-8);
    const T p2 = (K13 * q0 - K76 * q1) + K116 * q2;
    const T p1 = (K56 * q2 - K16 * q1) + K13 * q3;
    const T p0 = (K13 * q2 + K56 * q3) - K16 * q4;
    const T s2 = (t0 - T(2) * t1) + t2, d2 = (t0 - T(4) * t1) + T(3) * t2;
    const T s1 = (t1 - T(2) * t2) + t3, d1 = t1 - t3;
    const T s0 = (t2 - T(2) * t3) + t4, d0 = (T(3) * t2 - T(4) * t3) + t4;
    const T b2 = K1312 * (s2 * s2) + T(0.25) * (d2 * d2);
    const T b1 = K1312 * (s1 * s1) + T(0.25) * (d1 * d1);
    const T b0 = K1312 * (s0 * s0) + T(0.25) * (d0 * d0);
    const T tau = abs_of(b0 - b2);
    const T r0 = tau / (b0 + EPS), r1 = tau / (b1 + EPS), r2 = tau / (b2 + EPS);
    const T a0 = K310 * (T(1) + r0 * r0), a1 = K35 * (T(1) + r1 * r1), a2 = K110 * (T(1) + r2 * r2);
    return ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2);
}

// W5V(q0..q4; a0..a4; b0..b4) of include/tripolar_hip_weno_vs.h (the VelocityStencil form of k_weno_momentum_advection,
// tpg_weno_vorticity_kernel.hpp), the ONE definition: R above with each smoothness indicator the halved sum of the indicator of a0..a4 and
// the indicator of b0..b4, the candidates p2, p1, p0 from q0..q4.  W5V(q; q; q) is R(q) bit for bit where x + x and T(0.5) * (2x) are exact
// [recalled: Oceananigans' biased WENO weights for VelocityStencil -- the smoothness indicators of the tangential stencils of the two
// velocities averaged onto (Face, Face), summed and halved (beta_sum); parity unpinned, like every operator here]
template <typename T>
__device__ __forceinline__ T weno_face_vs(T q0, T q1, T q2, T q3, T q4, T a0, T a1, T a2, T a3, T a4, T b0, T b1, T b2, T b3, T b4)
{
    constexpr T K13 = T(1) / T(3), K76 = T(7) / T(6), K116 = T(11) / T(6), K56 = T(5) / T(6), K16 = T(1) / T(6);
    constexpr T K1312 = T(13) / T(12), K310 = T(3) / T(10), K35 = T(3) / T(5), K110 = T(1) / T(10);
    constexpr T EPS = T(1e-8);
    const T p2 = (K13 * q0 - K76 * q1) + K116 * q2;
    const T p1 = (K56 * q2 - K16 * q1) + K13 * q3;
    const T p0 = (K13 * q2 + K56 * q3) - K16 * q4;
    const T sA2 = (a0 - T(2) * a1) + a2, dA2 = (a0 - T(4) * a1) + T(3) * a2;
    const T sA1 = (a1 - T(2) * a2) + a3, dA1 = a1 - a3;
    const T sA0 = (a2 - T(2) * a3) + a4, dA0 = (T(3) * a2 - T(4) * a3) + a4;
    const T sB2 = (b0 - T(2) * b1) + b2, dB2 = (b0 - T(4) * b1) + T(3) * b2;
    const T sB1 = (b1 - T(2) * b2) + b3, dB1 = b1 - b3;
    const T sB0 = (b2 - T(2) * b3) + b4, dB0 = (T(3) * b2 - T(4) * b3) + b4;
    const T bA2 = K1312 * (sA2 * sA2) + T(0.25) * (dA2 * dA2), bB2 = K1312 * (sB2 * sB2) + T(0.25) * (dB2 * dB2);
    const T bA1 = K1312 * (sA1 * sA1) + T(0.25) * (dA1 * dA1), bB1 = K1312 * (sB1 * sB1) + T(0.25) * (dB1 * dB1);
    const T bA0 = K1312 * (sA0 * sA0) + T(0.25) * (dA0 * dA0), bB0 = K1312 * (sB0 * sB0) + T(0.25) * (dB0 * dB0);
    const T s2 = T(0.5) * (bA2 + bB2), s1 = T(0.5) * (bA1 + bB1), s0 = T(0.5) * (bA0 + bB0);
    const T tau = abs_of(s0 - s2);
    const T r0 = tau / (s0 + EPS), r1 = tau / (s1 + EPS), r2 = tau / (s2 + EPS);
    const T w0 = K310 * (T(1) + r0 * r0), w1 = K35 * (T(1) + r1 * r1), w2 = K110 * (T(1) + r2 * r2);
    return ((w0 * p0 + w1 * p1) + w2 * p2) / ((w0 + w1) + w2);
}

// R3(q0, q1, q2) of include/tripolar_hip_weno_xyz.h, the face value of order three: q1 is the upwind cell, q2 the downwind one
template <typename T>
__device__ __forceinline__ T weno_face3(T q0, T q1, T q2)
{
    constexpr T K23 = T(2) / T(3), K13 = T(1) / T(3);
    constexpr T EPS = T(1e-8);
    const T p1 = T(1.5) * q1 - T(0.5) * q0;
    const T p0 = T(0.5) * (q1 + q2);
    const T e1 = q1 - q0, b1 = e1 * e1;
    const T e0 = q2 - q1, b0 = e0 * e0;
    const T tau = abs_of(b0 - b1);
    const T r0 = tau / (b0 + EPS), r1 = tau / (b1 + EPS);
    const T a0 = K23 * (T(1) + r0 * r0), a1 = K13 * (T(1) + r1 * r1);
    return (a0 * p0 + a1 * p1) / (a0 + a1);
}

// the order table of that header's z-faces: face f = 1 .. Nz + 1 lies between the levels f - 1 and f, and its order depends on its distance
// from the nearer wall only -- 0: the centred mean (WENO_Z_CENTRED), 1: order 1, 2: order 3, 3 and more: order 5
enum { WENO_Z_CENTRED = 0, WENO_Z_ORDER1 = 1, WENO_Z_ORDER3 = 2, WENO_Z_ORDER5 = 3 };
__host__ __device__ __forceinline__ int weno_z_face_class(int f, int Nz)
{
    const int dist = f - 1 < Nz + 1 - f ? f - 1 : Nz + 1 - f;
    return dist < WENO_Z_ORDER5 ? dist : WENO_Z_ORDER5;
}

}  // namespace
