// hung_solve: the shortest-augmenting-path Hungarian method on integer costs for ONE wavefront, shared by the track scorer
// (mot.hip) and the tracker's optimal association (track.hip).  Lanes own columns (column j is lane j % 64), a row step is one
// wave minimum over (minv, column), and the costs are formed on the fly by the caller's functor.  Every decision is an integer
// comparison, so no order of evaluation can change it.
#pragma once
#include "common.h"

constexpr int MOT_WAVE = 64;
constexpr int64_t MOT_ONE = 65536, MOT_BIG = 1ll << 27, MOT_INF = 1ll << 60;

template <int N>
struct HungLds {
    static_assert(N <= 2048, "a lane's used columns are one 32-bit mask");
    int64_t u[N], v[N], minv[N];                 // row and column potentials, the reduced cost of the best way into a column
    int32_t way[N], p[N];                        // the column before it on that way (-1: the inserted row); the row of a column
};

__device__ __forceinline__ int64_t wave_min(int64_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t o = __shfl_xor(x, off);
        x = o < x ? o : x;
    }
    return x;
}

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off));
    return x;
}

__device__ __forceinline__ int64_t wave_sum(int64_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// What orders the solver's LDS traffic between its steps.  HungBlockSync is the barrier of a one-wave workgroup; HungWaveSync is
// for one wavefront of a larger workgroup, where a workgroup barrier would wait for waves that never come: the LDS serves the
// operations of one wave in order, so it only has to wait for them and keep the compiler from moving accesses across it.
struct HungBlockSync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
struct HungWaveSync {
    __device__ __forceinline__ void operator()() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

// The minimum-cost assignment of n rows to m columns, n <= m <= N, cost(i, j) >= 0 an int64: afterwards s.p[j] is the row of
// column j or -1.  Rows are inserted in ascending order; inside an augmentation the next column is the unused column of least
// minv, the lowest index on a tie.  One wavefront; every branch is wave-uniform (the barriers are those of `sync`).
template <int N, typename Cost, typename Sync = HungBlockSync>
__device__ void hung_solve(HungLds<N> &s, int n, int m, const Cost &cost, int lane, const Sync &sync = Sync()) {
    for (int j = lane; j < m; j += MOT_WAVE) {
        s.v[j] = 0;
        s.p[j] = -1;
    }
    for (int i = lane; i < n; i += MOT_WAVE) s.u[i] = 0;
    sync();
    for (int i = 0; i < n; ++i) {
        for (int j = lane; j < m; j += MOT_WAVE) s.minv[j] = MOT_INF;
        uint32_t used = 0;                                             // bit k: column lane + 64k
        int j0 = -1;
        for (;;) {
            if (j0 >= 0 && (j0 & 63) == lane) used |= 1u << (j0 >> 6);
            const int i0 = j0 < 0 ? i : s.p[j0];
            const int64_t ui = s.u[i0];
            int64_t best = MOT_INF;
            int best_j = 0x7fffffff;
            for (int j = lane, k = 0; j < m; j += MOT_WAVE, ++k) {
                if ((used >> k) & 1u) continue;
                const int64_t cur = cost(i0, j) - ui - s.v[j];
                int64_t mv = s.minv[j];
                if (cur < mv) {
                    mv = cur;
                    s.minv[j] = cur;
                    s.way[j] = j0;
                }
                if (mv < best) {
                    best = mv;
                    best_j = j;
                }
            }
            const int64_t delta = wave_min(best);
            const int j1 = wave_min(best == delta ? best_j : 0x7fffffff);
            for (int j = lane, k = 0; j < m; j += MOT_WAVE, ++k) {
                if ((used >> k) & 1u) {
                    s.u[s.p[j]] += delta;                              // p is one-to-one: every lane its own row
                    s.v[j] -= delta;
                } else {
                    s.minv[j] -= delta;
                }
            }
            if (lane == 0) s.u[i] += delta;                            // the inserted row: not in p yet
            sync();
            if (j1 >= m) return;                                       // n <= m leaves an unused column: never taken
            j0 = j1;
            if (s.p[j0] < 0) break;
        }
        if (lane == 0) {
            do {
                const int j1 = s.way[j0];
                s.p[j0] = j1 < 0 ? i : s.p[j1];
                j0 = j1;
            } while (j0 >= 0);
        }
        sync();
    }
}
