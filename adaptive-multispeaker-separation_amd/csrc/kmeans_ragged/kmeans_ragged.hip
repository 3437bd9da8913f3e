// Hard k-means over segments of different numbers of points (include/ams_kmeans_ragged.h): libams_kmeans_ragged.so.
//
// The passes ARE the tuned hard passes of libams_hip.so: the kernels of csrc/kmeans_hard.h instantiated with the geometry KmRagged where
// csrc/kmeans.hip instantiates them with KmDense, so every running sum sees the same terms in the same order; only the index arithmetic,
// which the geometry states, differs: (segment, chunk, column) from the host-built work table, the segment's length, chunk count and
// place among the partial rows from p_off / g_off.  One launch per pass whatever the number of segments; only KmRagged::pair's (E, C).
#include "../kmeans_hard.h"
#include "../../../include/ams_kmeans_ragged.h"

thread_local int g_ams_last_hip_error = 0;      // (common.h: this library keeps its own)

namespace {

// centroids[r, c, :] = xn[p_off[r / tries] + idx[r, c], :]
__global__ void kmr_init_kernel(const float* __restrict__ xn, const long* __restrict__ p_off, const int32_t* __restrict__ idx,
                                float* __restrict__ cent, long n, int C, int E, int tries) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e = (int)(i % E);
    const long rc = i / E;
    const int r = (int)(rc / C);
    cent[i] = xn[(p_off[r / tries] + idx[rc]) * E + e];
}

bool kmr_sizes(int R, int tries, long Gtot) { return R >= 1 && tries >= 1 && Gtot >= R && 4 * Gtot * (long)tries < (1L << 31); }

// five tries per read of the points: E = 40, C = 2, tries a multiple of 5, 32-bit buffer offsets inside every segment
bool kmr_tries_kernel(int tries, long Pmax, int E, int C) { return E == 40 && C == 2 && tries % TQ == 0 && Pmax * E * 4 < (1L << 31); }

KmRagged::Args kmr_args(const float* xn, const float* w, const int32_t* tab, const long* p_off, const long* g_off, const float* cent, int R,
                int tries, long Gtot) {
    KmRagged::Args a{};
    a.xn = xn; a.w = w; a.cent = cent; a.b = R; a.tries = tries; a.beta = -1.0f; a.one = 1.0f;
    a.tab = tab; a.p_off = p_off; a.g_off = g_off; a.Gtot = (int)Gtot;
    return a;
}

KmRagged::TArgs kmr_targs(const float* xn, const float* w, const int32_t* tab, const long* p_off, const long* g_off, const float* cent, int R,
                 int tries) {
    KmRagged::TArgs k{};
    k.xn = xn; k.w = w; k.cent = cent; k.b = R; k.tries = tries;
    k.tab = tab; k.p_off = p_off; k.g_off = g_off;
    return k;
}

}  // namespace

extern "C" {

int ams_kmr_abi_version(void) { return 1; }

long ams_kmr_chunks(const int64_t* p_off, int R) {
    if (!p_off || R < 1 || p_off[0] != 0) return -1;
    long G = 0;
    for (int r = 0; r < R; ++r) {
        const long P = p_off[r + 1] - p_off[r];
        if (P < 1) return -1;
        G += (P + CHUNK_HARD - 1) / CHUNK_HARD;
        if (4 * G >= (1L << 31)) return -1;
    }
    return G;
}

ams_status ams_kmr_tables(const int64_t* p_off, int R, int64_t* g_off, int32_t* tab) {
    AMS_REQUIRE(g_off && tab && ams_kmr_chunks(p_off, R) > 0);
    long G = 0;
    for (int r = 0; r < R; ++r) {
        g_off[r] = G;
        const long Gr = (p_off[r + 1] - p_off[r] + CHUNK_HARD - 1) / CHUNK_HARD;
        for (long g = 0; g < Gr; ++g)
            for (int k = 0; k < 4; ++k) {
                int32_t* e = tab + (4 * (G + g) + k) * 4;
                e[0] = r; e[1] = (int32_t)g; e[2] = k; e[3] = 0;
            }
        G += Gr;
    }
    g_off[R] = G;
    return AMS_OK;
}

size_t ams_kmr_workspace_bytes(int R, int tries, long Gtot, int E, int C) {
    if (!KmRagged::pair(E, C) || !kmr_sizes(R, tries, Gtot)) return 0;
    return sizeof(float) * (size_t)tries * 4 * (size_t)Gtot * C * (E + 1);
}

ams_status ams_kmr_init(const float* xn, const int64_t* p_off, const int32_t* init_idx, float* centroids, int R, int tries, int E, int C,
                        void* stream) {
    AMS_REQUIRE(xn && p_off && init_idx && centroids && R >= 1 && tries >= 1 && KmRagged::pair(E, C));
    const long n = (long)R * tries * C * E;
    AMS_REQUIRE(n < (1L << 31) * 256);
    hipLaunchKernelGGL(kmr_init_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, xn, (const long*)p_off,
                       init_idx, centroids, n, C, E, tries);
    return ams_check_launch();
}

ams_status ams_kmr_iterate(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                           const float* cent_in, float* cent_out, int R, int tries, long Gtot, long Pmax, int E, int C, void* ws,
                           size_t ws_bytes, void* tickets, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent_in && cent_out && ws && tickets && KmRagged::pair(E, C) && kmr_sizes(R, tries, Gtot) &&
                Pmax >= 1);
    if (ws_bytes < ams_kmr_workspace_bytes(R, tries, Gtot, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    if (kmr_tries_kernel(tries, Pmax, E, C)) {
        KmRagged::TArgs k = kmr_targs(xn, w, tab, (const long*)p_off, (const long*)g_off, cent_in, R, tries);
        k.part = (float*)ws; k.tickets = (unsigned*)tickets; k.fin_out = cent_out;
        const dim3 grid((unsigned)(4 * Gtot * (tries / TQ)));       // (try group, unit of the table)
        if (w) hipLaunchKernelGGL((kmeans_hard_tries_kernel<KmRagged, true>), grid, dim3(640), KT_LDS_BYTES, st, k);
        else hipLaunchKernelGGL((kmeans_hard_tries_kernel<KmRagged, false>), grid, dim3(640), KT_LDS_BYTES, st, k);
        return ams_check_launch();
    }
    KmRagged::Args a = kmr_args(xn, w, tab, (const long*)p_off, (const long*)g_off, cent_in, R, tries, Gtot);
    a.part = (float*)ws; a.tickets = (unsigned*)tickets; a.fin_out = cent_out;
    if (C > 4) return launch_grouped<KmRagged>(a, E, C, st);
    return launch_pass<KmRagged, HARD_ACC>(a, R * tries, E, C, st);
}

ams_status ams_kmr_inertia(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                           const float* cent, float* inertia, int R, int tries, long Gtot, long Pmax, int E, int C, void* ws,
                           size_t ws_bytes, void* tickets, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent && inertia && ws && tickets && KmRagged::pair(E, C) && kmr_sizes(R, tries, Gtot) && Pmax >= 1);
    if (ws_bytes < ams_kmr_workspace_bytes(R, tries, Gtot, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    if (kmr_tries_kernel(tries, Pmax, E, C)) {
        KmRagged::TArgs k = kmr_targs(xn, w, tab, (const long*)p_off, (const long*)g_off, cent, R, tries);
        k.part = (float*)ws; k.tickets = (unsigned*)tickets; k.fin_out = inertia;
        const dim3 grid((unsigned)(2 * Gtot * (tries / TQ)));       // (try group, column pair of the table)
        if (w) hipLaunchKernelGGL((kmeans_hard_tries_final_kernel<KmRagged, true>), grid, dim3(640), 2 * 128 * 40 * sizeof(float), st, k);
        else hipLaunchKernelGGL((kmeans_hard_tries_final_kernel<KmRagged, false>), grid, dim3(640), 2 * 128 * 40 * sizeof(float), st, k);
        return ams_check_launch();
    }
    KmRagged::Args a = kmr_args(xn, w, tab, (const long*)p_off, (const long*)g_off, cent, R, tries, Gtot);
    a.part = (float*)ws; a.tickets = (unsigned*)tickets; a.fin_out = inertia;
    return launch_pass<KmRagged, HARD_FINAL>(a, R * tries, E, C, st);
}

ams_status ams_kmr_select(const float* inertia, const float* centroids, int32_t* best, float* selected, int R, int tries, int E, int C,
                          void* stream) {
    AMS_REQUIRE(inertia && centroids && best && selected && R >= 1 && tries >= 1 && KmRagged::pair(E, C));
    hipLaunchKernelGGL(kmeans_select_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, inertia, centroids, best, selected, R, tries, C * E);
    return ams_check_launch();
}

ams_status ams_kmr_labels(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                          const float* cent, int32_t* labels, int R, long Gtot, int E, int C, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent && labels && KmRagged::pair(E, C) && kmr_sizes(R, 1, Gtot));
    KmRagged::Args a = kmr_args(xn, w, tab, (const long*)p_off, (const long*)g_off, cent, R, 1, Gtot);
    a.labels = labels;                                              // (no partial sums, no tickets: HARD_LABELS stores labels only)
    return launch_pass<KmRagged, HARD_LABELS>(a, R, E, C, (hipStream_t)stream);
}

}  // extern "C"
