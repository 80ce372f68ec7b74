// gcc_amd/csrc/task_common.h -- the kit the downstream-task files share (simsearch.hip, svc.hip, logreg.hip, prone.hip,
// graphwave.hip; graph_build.hip and graph_tables.hip take the host scaffold): THE implementation of the fixed-order row sum of include/gcc_amd.h ("ORDER OF A ROW'S SUM"), the CSR guards, the
// workgroup sum, the float64 Gram tile on v_mfma_f64_16x16x4_f64, and the host scaffold of an entry point (workspace carving, the
// NULL / workspace checks with their messages, the launch check).  Everything is file-local: every source file is its own
// translation unit, in the product and in the emulator build alike.
#pragma once
#include "host_common.h"

#include <initializer_list>

namespace {

// ---------------------------------------------------------------- device
// sums of 2^l items at level l, for C columns: push() adds item number t (t items came before), fold() adds what is left from the
// lowest level up, onto s when `have`.  Every loop has constant bounds and is unrolled, so every index is a constant.  (push() tests
// the carry once per level, outside the column loop: tested per column, pr_spmm_kernel takes 72 VGPRs for 58 and loses a wave per
// SIMD.)
template <int L, int C> struct SumCounter {
    double v[C][L];
    __device__ __forceinline__ SumCounter()
    {
#pragma unroll
        for (int k = 0; k < C; ++k)
#pragma unroll
            for (int l = 0; l < L; ++l) v[k][l] = 0.0;
    }
    __device__ __forceinline__ void push(int t, const double (&item)[C])
    {
        double c[C];
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = item[k];
        bool go = true;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            if (!go) continue;
            if ((t >> l) & 1) {
#pragma unroll
                for (int k = 0; k < C; ++k) c[k] = v[k][l] + c[k];
            } else {
#pragma unroll
                for (int k = 0; k < C; ++k) v[k][l] = c[k];
                go = false;
            }
        }
    }
    __device__ __forceinline__ void fold(int m, bool have, double (&s)[C]) const
    {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            if (!((m >> l) & 1)) continue;
#pragma unroll
            for (int k = 0; k < C; ++k) s[k] = have ? v[k][l] + s[k] : v[k][l];
            have = true;
        }
    }
    // the sum of the m items pushed (one column)
    __device__ __forceinline__ double fold(int m) const
    {
        static_assert(C == 1, "one column");
        double s[1] = {0.0};
        fold(m, false, s);
        return s[0];
    }
};

// the entries of row i; a row_ptr that does not fit gives an empty row (the caller's first kernel reports it)
__device__ __forceinline__ bool csr_row_range(const int32_t *rp, int nnz, int i, int &b, int &e)
{
    b = rp[i];
    e = rp[i + 1];
    if (b < 0 || e < b || e > nnz) {
        b = e = 0;
        return false;
    }
    return true;
}
// row_ptr's two ends, looked at by the first and the last row
__device__ __forceinline__ bool csr_ends_ok(const int32_t *rp, int n, int nnz, int i)
{
    return !(i == 0 && rp[0] != 0) && !(i == n - 1 && rp[n] != nnz);
}
// entry q of row i, whose entries begin at b: outside [0, n), a self loop, or below the entry before it
__device__ __forceinline__ bool csr_entry_bad(const int32_t *ci, int b, int q, int i, int n)
{
    const int j = ci[q], before = q > b ? ci[q - 1] : -1;
    return (unsigned)j >= (unsigned)n || j == i || before > j;
}

// sum over the workgroup in one fixed order: wave sums, then the waves in wave order (every thread gets the result)
template <int kWaves> __device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < kWaves; ++w) r += red[w];
    __syncthreads();
    return r;
}

// tile t of the upper triangle, rows first: (0,0), (0,1), ..., (0,T-1), (1,1), ...
__device__ __forceinline__ void tri_tile_of(int t, int T, int &ti, int &tj)
{
    ti = 0;
    for (int width = T; t >= width; --width) { t -= width; ++ti; }
    tj = ti + t;
}
__host__ __device__ inline int tri_tile_index(int ti, int tj, int T) { return ti * T - ti * (ti - 1) / 2 + (tj - ti); }

// One 16 x 16 tile of sum over the rows [r0, r1) of a[row] b[row]^T on v_mfma_f64_16x16x4_f64, by a workgroup of kGramWaves waves
// (all of them call): four rows per instruction, a wave takes the row groups wv, wv + 4, ... and the waves are added in wave
// order.  Lane (jl = lane & 15, q = lane >> 4) passes A[jl][q] = load_a(row, in) and B[q][jl] = load_b(row, in) of the group's row
// q; `in`: row < r1 (a row past the end must give 0 on one side at least).  red: [kGramWaves][256] of LDS.
// -> the tile in row-major order, entry threadIdx.x
constexpr int kGramWaves = 4;
template <class LoadA, class LoadB>
__device__ __forceinline__ double gram_tile_f64(int r0, int r1, LoadA load_a, LoadB load_b, double (*red)[256])
{
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6, jl = lane & 15, q = lane >> 4;
    const f64x4 z4 = {0.0, 0.0, 0.0, 0.0};
    f64x4 acc0 = z4, acc1 = z4;
    for (int rb = r0 + 4 * wv; rb < r1; rb += 8 * kGramWaves) {
        const int ra = rb + q, rc = rb + 4 * kGramWaves + q;
        const bool ina = ra < r1, inc = rc < r1;
        const double xa0 = load_a(ra, ina), xb0 = load_b(ra, ina), xa1 = load_a(rc, inc), xb1 = load_b(rc, inc);
        acc0 = mfma_16x16x4_f64(xa0, xb0, acc0);
        acc1 = mfma_16x16x4_f64(xa1, xb1, acc1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wv][(q + 4 * r) * 16 + jl] = acc0[r] + acc1[r];     // c/d[r] = C[q + 4 r][jl]
    __syncthreads();
    return ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---------------------------------------------------------------- host
// a running offset into the workspace: every piece begins on a multiple of 256 bytes
struct Carve {
    int64_t off = 0;
    int64_t take(int64_t bytes)
    {
        const int64_t at = off;
        off = (off + bytes + 255) & ~(int64_t)255;
        return at;
    }
    int64_t total() const { return off; }
};

template <class T> T *ws_at(void *workspace, int64_t off) { return reinterpret_cast<T *>(static_cast<unsigned char *>(workspace) + off); }

// -1 and the name of the first member that is NULL where it is needed
struct Member {
    const void *ptr;
    const char *name;
    bool needed = true;
};
int null_member(const char *who, std::initializer_list<Member> members)
{
    for (const Member &m : members)
        if (m.needed && !m.ptr) {
            snprintf(g_err, kErrLen, "%s: %s is NULL", who, m.name);
            return -1;
        }
    return 0;
}

// -8: the workspace is smaller than `query` asks for; -9: it is not aligned
int check_workspace(const char *who, const char *query, const void *workspace, int64_t bytes, int64_t need)
{
    if (!workspace || bytes < need) {
        snprintf(g_err, kErrLen, "%s: workspace_bytes %lld is less than %s (%lld)", who, (long long)(workspace ? bytes : 0), query,
                 (long long)need);
        return -8;
    }
    if (((uintptr_t)workspace & 15) != 0) {
        snprintf(g_err, kErrLen, "%s: workspace must be aligned to 16 bytes", who);
        return -9;
    }
    return 0;
}

// what an entry point returns after its launches
int launched() { return hipGetLastError() == hipSuccess ? 0 : -10; }

}  // namespace
