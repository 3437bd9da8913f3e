// Live streams (include/ams_stream.h): the stitcher with its past carried in a state buffer on the device.
// A library of its own (libams_stream.so): the other headers and libraries are untouched.  Built with -ffp-contract=off.  The border sums,
// the search and the fade are ../stitch/stitch_core.h's, the header that stitch.hip compiles too; what is here is where an operand lies
// (the row before a stream's first row of a push is the tail the state carries) and where a workgroup finds its stream (a table the
// caller built on the host; grid.z or grid.y is the entry).  Launch counts do not depend on the number of streams.  No MFMA, no
// atomics, no scratch; no launch reads state that another workgroup of the same launch writes.
#include "../../../include/ams_stream.h"
#include "../stitch/stitch_core.h"

namespace {

constexpr int E = AMS_STREAM_ENTRY;
constexpr int TRK_WORDS = 8;          // words of trk per slot of the state

long g_launches = 0;

inline ams_status check_launch() {
    ++g_launches;
    return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED;
}
inline int up4(int a) { return (a + 3) / 4 * 4; }
inline bool shape_ok(int slots, int S, int L, int H) { return slots >= 1 && slots <= 65535 && sources_ok(S) && geometry_ok(L, H); }
inline bool push_ok(int slots, int n, int rows, int max_rows) {
    return n >= 1 && n <= slots && rows >= 0 && max_rows >= 0 && max_rows <= rows && max_rows <= 65535 && (long)rows <= 65535L * n;
}

// the state: pending [slots, Lp], tail [slots, S, Vp], trk [slots, TRK_WORDS]
struct State {
    float* pend;
    float* tail;
    int* trk;
    int Lp, Vp;
};
inline State carve(void* state, int slots, int S, int L, int H) {
    State s;
    s.Lp = up4(L);
    s.Vp = up4(L - H);
    s.pend = (float*)state;
    s.tail = s.pend + (size_t)slots * s.Lp;
    s.trk = (int*)(s.tail + (size_t)slots * S * s.Vp);
    return s;
}

// one entry of the table, and whether its numbers stay inside the buffers of this call
struct Entry {
    int slot, x_off, k, pend, rows, row0, out_off, m, flags;
};
__device__ __forceinline__ Entry entry_of(const int* __restrict__ table, int s) {
    const int* t = table + (long)s * E;
    Entry e;
    e.slot = t[0]; e.x_off = t[1]; e.k = t[2]; e.pend = t[3]; e.rows = t[4]; e.row0 = t[5]; e.out_off = t[6]; e.m = t[7]; e.flags = t[8];
    return e;
}
__device__ __forceinline__ bool entry_ok(const Entry& e, int slots, int rows_total, int L) {
    return e.slot >= 0 && e.slot < slots && e.k >= 0 && e.pend >= 0 && e.pend < L && e.rows >= 0 && e.row0 >= 0 && e.x_off >= 0 &&
           (long)e.row0 + e.rows <= rows_total && e.out_off >= 0 && e.m >= 0;
}

// ------------------------------------------------------------------ reset
__global__ __launch_bounds__(256) void reset_kernel(State st, int S, int first) {
    const int slot = first + blockIdx.x;
    float* const p = st.pend + (long)slot * st.Lp;
    for (int i = threadIdx.x; i < st.Lp; i += 256) p[i] = 0.f;
    float* const t = st.tail + (long)slot * S * st.Vp;
    for (int i = threadIdx.x; i < S * st.Vp; i += 256) t[i] = 0.f;
    if (threadIdx.x < TRK_WORDS) st.trk[(long)slot * TRK_WORDS + threadIdx.x] = threadIdx.x;
}

// ------------------------------------------------------------------ feed
// sample v of what the stream holds from chunk D on: its pending samples, then its new ones, then zeros
__device__ __forceinline__ float held(const float* __restrict__ pend, const float* __restrict__ x, const Entry& e, long v) {
    if (v < e.pend) return pend[v];
    v -= e.pend;
    return v < e.k ? x[e.x_off + v] : 0.f;
}

__global__ __launch_bounds__(256) void cut_kernel(State st, const int* __restrict__ table, const float* __restrict__ x, long x_total,
                                                  float* __restrict__ mix, int slots, int rows_total, int L, int H) {
    const Entry e = entry_of(table, blockIdx.z);
    if (!entry_ok(e, slots, rows_total, L) || (long)e.x_off + e.k > x_total) return;
    const float* const pend = st.pend + (long)e.slot * st.Lp;
    for (int j = blockIdx.y; j < e.rows; j += gridDim.y) {
        float* const row = mix + (long)(e.row0 + j) * L;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int l = blockIdx.x * 1024 + q * 256 + threadIdx.x;
            if (l >= L) break;
            row[l] = held(pend, x, e, (long)j * H + l);
        }
    }
}

// the samples from (rows) H on become the pending ones.  With a row, those still inside what WAS pending come from the last row of mix
// (this launch writes the pending buffer, so it does not read it); without one, the new samples go behind what is pending
__global__ __launch_bounds__(256) void keep_kernel(State st, const int* __restrict__ table, const float* __restrict__ x, long x_total,
                                                   const float* __restrict__ mix, int slots, int rows_total, int L, int H) {
    const Entry e = entry_of(table, blockIdx.y);
    if (!entry_ok(e, slots, rows_total, L) || (long)e.x_off + e.k > x_total) return;
    float* const pend = st.pend + (long)e.slot * st.Lp;
    const long start = (long)e.rows * H;                              // of the new pending samples, in `held` positions
    const long left = (long)e.pend + e.k - start;                     // how many there are: < L by the plan; <= 0 after a closing row
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = blockIdx.x * 1024 + q * 256 + threadIdx.x;
        if (i >= L || i >= left) break;
        const long v = start + i;
        if (v >= e.pend) pend[i] = x[e.x_off + (v - e.pend)];
        else if (e.rows > 0) pend[i] = mix[(long)(e.row0 + e.rows - 1) * L + (v - (long)(e.rows - 1) * H)];
    }
}

// ------------------------------------------------------------------ border table
// the border in front of every row: the row before it is the carried tail (rows Vp apart) for a push's first row, est's otherwise
template <int S, bool VEC>
__global__ __launch_bounds__(256) void stats_kernel(State st, const int* __restrict__ table, const float* __restrict__ est,
                                                    float* __restrict__ part, int slots, int rows_total, int L, int H) {
    const Entry e = entry_of(table, blockIdx.z);
    if (!entry_ok(e, slots, rows_total, L)) return;                       // the same for the whole workgroup
    const int V = L - H, nslab = gridDim.x, slab = blockIdx.x;
    const int v0 = slab * SLAB, v1 = min(V, v0 + SLAB);
    for (int j = blockIdx.y; j < e.rows; j += gridDim.y) {
        if (j == 0 && (e.flags & AMS_STREAM_FIRST)) continue;             // chunk 0: no border in front of it
        const long c = e.row0 + j;
        const float* const tail = j == 0 ? st.tail + (long)e.slot * S * st.Vp : est + (c - 1) * S * L + H;
        border_sums<S, VEC>(tail, j == 0 ? st.Vp : L, est + c * S * L, L, v0, v1, part + (c * nslab + slab) * (S * S));
    }
}

// ------------------------------------------------------------------ border permutations and tracks
// One workgroup per stream walks the stream's rows in order: Q of the row's border (the slab sums in slab order), the search,
// trk <- rel[trk].  tw [rows + n, S]: entry s owns rows row0 + s .. row0 + s + rows of it: the carried trk, then the trk of every row.
__global__ __launch_bounds__(256) void track_kernel(State st, const int* __restrict__ table, const float* __restrict__ part,
                                                    const int* __restrict__ perms, int* __restrict__ tw, float* __restrict__ Q_rows,
                                                    int* __restrict__ trk_rows, int slots, int rows_total, int L, int nslab, int S, int P) {
    __shared__ float q[36];
    __shared__ float sc[256];
    __shared__ int sp[256];
    __shared__ int cur[TRK_WORDS];
    const Entry e = entry_of(table, blockIdx.x);
    if (!entry_ok(e, slots, rows_total, L)) return;
    const int SS = S * S, tid = threadIdx.x;
    int* const strk = st.trk + (long)e.slot * TRK_WORDS;
    int* const mine = tw + ((long)e.row0 + blockIdx.x) * S;
    if (tid < S) {
        const int k = (e.flags & AMS_STREAM_FIRST) ? tid : strk[tid];
        cur[tid] = k;
        mine[tid] = k;
    }
    __syncthreads();
    for (int j = 0; j < e.rows; ++j) {
        const long c = e.row0 + j;
        int win = 0;
        if (j == 0 && (e.flags & AMS_STREAM_FIRST)) {                  // chunk 0: the identity, and a row of zeros for Q
            if (Q_rows && tid < SS) Q_rows[c * SS + tid] = 0.f;
        } else {
            if (tid < SS) {
                const float s = slab_fold(part + c * nslab * SS + tid, nslab, SS);
                q[tid] = s;
                if (Q_rows) Q_rows[c * SS + tid] = s;
            }
            __syncthreads();
            win = best_perm(q, sc, sp, perms, S, P);
        }
        int nxt = 0;
        if (tid < S) nxt = perms[(long)win * S + cur[tid]];              // (permutation 0 is the identity)
        __syncthreads();
        if (tid < S) {
            cur[tid] = nxt;
            mine[(long)(j + 1) * S + tid] = nxt;
            if (trk_rows) trk_rows[c * S + tid] = nxt;
        }
        __syncthreads();
    }
    if (tid < S) strk[tid] = cur[tid];
}

// ------------------------------------------------------------------ cross-fade
// output sample i of a stream's push: row j = i / H at p = i - j H, faded with the row before it (the carried tail for j == 0) where
// p < V; past the last row (a closing stream), the tail of the last row -- or the carried tail where the push has no row
__global__ __launch_bounds__(256) void ola_kernel(State st, const int* __restrict__ table, const float* __restrict__ est,
                                                  const int* __restrict__ tw, const float* __restrict__ w_head, float* __restrict__ out,
                                                  long out_stride, int slots, int rows_total, int S, int L, int H) {
    const Entry e = entry_of(table, blockIdx.y);
    if (!entry_ok(e, slots, rows_total, L) || (long)e.out_off + e.m > out_stride) return;
    const int k = blockIdx.z, V = L - H;
    const int* const mine = tw + ((long)e.row0 + blockIdx.y) * S;
    const float* const carried = st.tail + (long)e.slot * S * st.Vp;
    float* const orow = out + (long)k * out_stride + e.out_off;
    for (long b = blockIdx.x; b * 1024 < e.m; b += gridDim.x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long i = b * 1024 + q * 256 + threadIdx.x;
            if (i >= e.m) break;
            const long j = i / H;
            float r;
            if (j < e.rows) {
                const long p = i - j * H, c = e.row0 + j;
                r = est[(c * S + mine[(j + 1) * S + k]) * L + p];
                if (p < V && !(j == 0 && (e.flags & AMS_STREAM_FIRST))) {
                    const int kp = mine[j * S + k];
                    const float t = j == 0 ? carried[(long)kp * st.Vp + p] : est[((c - 1) * S + kp) * L + H + p];
                    r = fade(w_head[p], t, r);
                }
            } else {
                const long p = i - (long)e.rows * H;
                if (p >= V) break;                                         // (the plan never asks for it)
                const int kl = mine[(long)e.rows * S + k];
                r = e.rows > 0 ? est[(((long)e.row0 + e.rows - 1) * S + kl) * L + H + p] : carried[(long)kl * st.Vp + p];
            }
            orow[i] = r;
        }
    }
}

// tail <- est[last row, :, H .. L) in the model's own order
__global__ __launch_bounds__(256) void tail_kernel(State st, const int* __restrict__ table, const float* __restrict__ est, int slots,
                                                   int rows_total, int S, int L, int H) {
    const Entry e = entry_of(table, blockIdx.y);
    if (!entry_ok(e, slots, rows_total, L) || e.rows < 1) return;
    const int i = blockIdx.z, V = L - H;
    const float* const src = est + (((long)e.row0 + e.rows - 1) * S + i) * L + H;
    float* const dst = st.tail + ((long)e.slot * S + i) * st.Vp;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = blockIdx.x * 1024 + q * 256 + threadIdx.x;
        if (v >= V) break;
        dst[v] = src[v];
    }
}

}  // namespace

extern "C" {

int ams_stream_abi_version(void) { return 1; }

long ams_stream_launch_count(void) { return g_launches; }

size_t ams_stream_state_bytes(int slots, int S, int L, int H) {
    if (!shape_ok(slots, S, L, H)) return 0;
    return (size_t)slots * ((size_t)up4(L) + (size_t)S * up4(L - H) + TRK_WORDS) * sizeof(float);
}

ams_status ams_stream_reset(void* state, int slots, int S, int L, int H, int first, int count, void* stream) {
    STITCH_REQUIRE(state && aligned16(state) && shape_ok(slots, S, L, H));
    STITCH_REQUIRE(first >= 0 && count >= 1 && (long)first + count <= slots);
    hipLaunchKernelGGL(reset_kernel, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, carve(state, slots, S, L, H), S, first);
    return check_launch();
}

ams_status ams_stream_feed(void* state, int slots, int S, int L, int H, const int32_t* table, int n, int rows, int max_rows,
                           const float* x, long x_total, float* mix, void* stream) {
    STITCH_REQUIRE(state && aligned16(state) && table && x && (mix || rows == 0));
    STITCH_REQUIRE(shape_ok(slots, S, L, H) && push_ok(slots, n, rows, max_rows));
    STITCH_REQUIRE(x_total >= 0 && x_total < (1L << 31));
    const State st = carve(state, slots, S, L, H);
    hipStream_t hs = (hipStream_t)stream;
    const unsigned gx = (unsigned)cdiv(L, 1024);
    hipLaunchKernelGGL(cut_kernel, dim3(gx, (unsigned)(max_rows > 0 ? max_rows : 1), (unsigned)n), dim3(256), 0, hs, st, table, x, x_total,
                       mix, slots, rows, L, H);
    ams_status rc = check_launch();
    if (rc != AMS_OK) return rc;
    hipLaunchKernelGGL(keep_kernel, dim3(gx, (unsigned)n), dim3(256), 0, hs, st, table, x, x_total, mix, slots, rows, L, H);
    return check_launch();
}

size_t ams_stream_workspace_bytes(int n, int rows, int S, int L, int H) {
    if (n < 1 || rows < 0 || !sources_ok(S) || !geometry_ok(L, H)) return 0;
    return ((size_t)rows * (size_t)cdiv(L - H, SLAB) * (size_t)(S * S) + ((size_t)rows + n) * S) * sizeof(float);
}

ams_status ams_stream_absorb(void* state, int slots, int S, int L, int H, const int32_t* table, int n, int rows, int max_rows, long max_m,
                             const float* est, const int32_t* perms, int P, const float* w_head, float* out, long out_stride, void* ws,
                             size_t ws_bytes, float* Q_rows, int32_t* trk_rows, void* stream) {
    STITCH_REQUIRE(state && aligned16(state) && table && perms && w_head && out && ws && (est || rows == 0));
    STITCH_REQUIRE(shape_ok(slots, S, L, H) && push_ok(slots, n, rows, max_rows));
    STITCH_REQUIRE(max_m >= 0 && out_stride >= 1 && max_m <= out_stride && out_stride < (1L << 31) / S);
    STITCH_REQUIRE(perm_count_ok(S, P));
    STITCH_REQUIRE(ws_bytes >= ams_stream_workspace_bytes(n, rows, S, L, H));
    const State st = carve(state, slots, S, L, H);
    hipStream_t hs = (hipStream_t)stream;
    const int V = L - H, nslab = (int)cdiv(V, SLAB);
    float* const part = (float*)ws;
    int* const tw = (int*)(part + (size_t)rows * nslab * S * S);
    const unsigned gy = (unsigned)(max_rows > 0 ? max_rows : 1);
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est);
    const dim3 grid((unsigned)nslab, gy, (unsigned)n);
    ams_status rc = for_sources(S, [&](auto s) {
        if (vec) hipLaunchKernelGGL((stats_kernel<s(), true>), grid, dim3(256), 0, hs, st, table, est, part, slots, rows, L, H);
        else hipLaunchKernelGGL((stats_kernel<s(), false>), grid, dim3(256), 0, hs, st, table, est, part, slots, rows, L, H);
        return check_launch();
    });
    if (rc != AMS_OK) return rc;
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)n), dim3(256), 0, hs, st, table, part, perms, tw, Q_rows, trk_rows, slots, rows, L,
                       nslab, S, P);
    rc = check_launch();
    if (rc != AMS_OK) return rc;
    long gb = cdiv(max_m, 1024);
    gb = gb < 1 ? 1 : (gb > 4096 ? 4096 : gb);                          // a workgroup row walks the blocks b, b + gridDim.x, ...
    hipLaunchKernelGGL(ola_kernel, dim3((unsigned)gb, (unsigned)n, (unsigned)S), dim3(256), 0, hs, st, table, est, tw, w_head, out,
                       out_stride, slots, rows, S, L, H);
    rc = check_launch();
    if (rc != AMS_OK) return rc;
    hipLaunchKernelGGL(tail_kernel, dim3((unsigned)cdiv(V, 1024), (unsigned)n, (unsigned)S), dim3(256), 0, hs, st, table, est, slots, rows,
                       S, L, H);
    return check_launch();
}

}  // extern "C"
