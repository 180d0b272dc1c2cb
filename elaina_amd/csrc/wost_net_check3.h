// wost_net_check3.h -- included by wost_net.hip alone, below ensure_points(); the drivers call check3_forward / check3_train behind check3_on()
// WOST_NET_CHECK3=1 (developer self check, EXPERIMENTS 20): the half-precision training kernels of every Adam step launched three times
// on the same inputs, the three results compared word by word on the device; the counts go to stderr when the network is destroyed
__global__ void check3_kernel(const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t n, unsigned long long *out, uint32_t *log)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = a[i], y = b[i], z = c[i];
    if (x == y && y == z) return;
    const unsigned long long k = atomicAdd(&out[0], 1ull);
    atomicAdd(&out[1 + (y == z ? 0 : x == z ? 1 : x == y ? 2 : 3)], 1ull);
    if (log && k < 65536ull) log[k] = (uint32_t)i;
}
struct Check3 {
    bool on = false, asked = false;
    unsigned long long *dev = nullptr;       // [kernel 0 forward / 1 train][words differing, odd launch 0 1 2, all differ] + launches with a difference
    void *scratch[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t scratch_bytes[4] = {0, 0, 0, 0};
    unsigned long long steps = 0;
    uint32_t *log = nullptr;                 // word indices of the forward kernel's first 65 536 differing words
    int n_out = 33, variant = 0;             // variant: the value of WOST_NET_CHECK3, read once (2: a discarded launch in front of the forward kernel)
};
static Check3 g_check3;

// ---- what runs in FRONT of the three launches of the self check (WOST_NET_CHECK3_PRE, EXPERIMENTS 20 / 26) ----------------------
// The first-tile deviation of net_forward_h_kernel appears when the kernel follows a different kernel.  Two readings: a transient of
// the matrix pipe at the start of matrix work, or state the previous launch left behind (LDS is never cleared between launches, the
// instruction cache holds the previous kernel).  These kernels set up one or the other in front of chosen launches:
//   "lds"      every LDS byte of every CU filled with half-precision NaNs in front of ALL three launches
//   "lds23"    ... in front of launches 2 and 3 only (which never deviate as things stand)
//   "burn1"    a heavy matrix kernel of another kind in front of launch 1 (a warm matrix pipe, foreign LDS / instruction cache)
//   "icache23" the instruction caches invalidated in front of launches 2 and 3
__global__ __launch_bounds__(1024) void check3_lds_fill_kernel(uint32_t pattern, uint32_t n_words, uint32_t *sink)
{
    extern __shared__ uint32_t s_fill[];
    for (uint32_t i = threadIdx.x; i < n_words; i += blockDim.x) s_fill[i] = pattern;
    __syncthreads();
    if (s_fill[(threadIdx.x * 977u) % n_words] != pattern) atomicAdd(sink, 1u);
}
__global__ void check3_icache_kernel()
{
    asm volatile("s_icache_inv\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
}
__global__ __launch_bounds__(1024) void check3_burn_kernel(int iters, float *sink)
{
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    f32x16 acc[4];
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 16; ++j) acc[k][j] = 0.0f;
    const h4 a = {(_Float16)(threadIdx.x & 7), (_Float16)1.0f, (_Float16)0.5f, (_Float16)0.25f}, b = {(_Float16)1.0f, (_Float16)(threadIdx.x & 3), (_Float16)2.0f, (_Float16)0.125f};
    for (int i = 0; i < iters; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, acc[k], 0, 0, 0);
    float t = 0.0f;
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 16; ++j) t += acc[k][j];
    if (t == 12345.678f) sink[0] = t;
}
static uint32_t check3_pre_mask()
{
    // bit k (0..2): lds in front of launch k; bit 3: burn in front of launch 0; bits 4, 5: icache in front of launches 1 and 2
    static int mask = -1;
    if (mask < 0) {
        mask = 0;
        const char *e = std::getenv("WOST_NET_CHECK3_PRE");
        const std::string v = e ? e : "";
        if (v.find("lds23") != std::string::npos) mask |= 6;
        else if (v.find("lds") != std::string::npos) mask |= 7;
        if (v.find("burn1") != std::string::npos) mask |= 8;
        if (v.find("icache23") != std::string::npos) mask |= 48;
    }
    return (uint32_t)mask;
}
static void check3_pre(int launch, hipStream_t stream)
{
    const uint32_t m = check3_pre_mask();
    if (!m || !g_check3.dev) return;
    uint32_t *sink = reinterpret_cast<uint32_t *>(g_check3.dev + 15);
    if (m & (1u << launch)) {
        const uint32_t bytes = 156u * 1024u;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(check3_lds_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        hipLaunchKernelGGL(check3_lds_fill_kernel, dim3(512), dim3(1024), bytes, stream, 0x7e007e00u, bytes / 4u, sink);
    }
    if (launch == 0 && (m & 8u)) hipLaunchKernelGGL(check3_burn_kernel, dim3(512), dim3(1024), 0, stream, 400, reinterpret_cast<float *>(sink));
    if ((launch == 1 && (m & 16u)) || (launch == 2 && (m & 32u))) hipLaunchKernelGGL(check3_icache_kernel, dim3(4096), dim3(64), 0, stream);
}
static bool check3_on()
{
    if (!g_check3.asked) {
        g_check3.asked = true;
        const char *e = std::getenv("WOST_NET_CHECK3");
        g_check3.variant = e ? std::atoi(e) : 0;
        g_check3.on = g_check3.variant != 0;
        if (g_check3.on && (hipMalloc((void **)&g_check3.log, 65536 * 4) != hipSuccess || hipMalloc((void **)&g_check3.dev, 16 * sizeof(unsigned long long)) != hipSuccess ||
                            hipMemset(g_check3.dev, 0, 16 * sizeof(unsigned long long)) != hipSuccess))
            g_check3.on = false;
    }
    return g_check3.on;
}
static void *check3_scratch(int k, size_t bytes)
{
    if (g_check3.scratch_bytes[k] < bytes) {
        if (g_check3.scratch[k]) (void)hipFree(g_check3.scratch[k]);
        g_check3.scratch[k] = nullptr;
        if (hipMalloc(&g_check3.scratch[k], bytes) != hipSuccess) return nullptr;
        g_check3.scratch_bytes[k] = bytes;
    }
    return g_check3.scratch[k];
}
static void check3_compare(int kernel, const void *a, const void *b, const void *c, size_t bytes, hipStream_t stream)
{
    const size_t words = bytes / 4;
    hipLaunchKernelGGL(check3_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const uint32_t *>(a),
                       reinterpret_cast<const uint32_t *>(b), reinterpret_cast<const uint32_t *>(c), words, g_check3.dev + 8 * kernel, kernel == 0 ? g_check3.log : nullptr);
}
// the forward pass of a half-precision training step (outputs to h->d_out, encodings to h->d_acts) among its repeats
static int check3_forward(wost_net *h, const float *xy_dev, int n, hipStream_t stream)
{
    const size_t ob = (size_t)n * h->L.n_out * 4, eb = (size_t)((n + 31) / 32 * 2) * 2 * 64 * 8;
    uint2 *e1 = (uint2 *)check3_scratch(2, eb);      // the encodings of every launch but the real one
    // variant 2: a discarded launch in front (is it the launch that follows OTHER kernels that differs, whatever it computes?)
    float *o3 = h->L.dims == 2 && g_check3.variant == 2 ? (float *)check3_scratch(3, ob) : nullptr;
    if (o3 && e1) (void)launch_forward_h(h, h->params, h->params_h, xy_dev, n, nullptr, o3, (size_t)h->L.n_out, 1, e1, stream);
    check3_pre(0, stream);
    const int rc = launch_forward_h(h, h->params, h->params_h, xy_dev, n, nullptr, h->d_out, (size_t)h->L.n_out, 1, reinterpret_cast<uint2 *>(h->d_acts), stream);
    if (rc != WOST_OK) return rc;
    g_check3.n_out = h->L.n_out;
    float *o[2] = {(float *)check3_scratch(0, ob), (float *)check3_scratch(1, ob)};
    if (!(o[0] && o[1] && e1)) return WOST_OK;
    for (int rep = 0; rep < 2; ++rep) {
        check3_pre(1 + rep, stream);
        (void)launch_forward_h(h, h->params, h->params_h, xy_dev, n, nullptr, o[rep], (size_t)h->L.n_out, 1, e1, stream);
    }
    check3_compare(0, h->d_out, o[0], o[1], ob, stream);
    ++g_check3.steps;
    return WOST_OK;
}
// two repeats of the net_train_h_kernel launch that backward_pass() has just issued (same grid, LDS size and delta scale 2^k)
static void check3_train(wost_net *h, int n, unsigned gridb, size_t lds, int k, hipStream_t stream)
{
    const NetLayout &L = h->L;
    if (L.dims != 2) return;
    const size_t db = (size_t)n * L.enc * 4, pb = (size_t)gridb * L.n_mlp * 4;
    float *d1 = (float *)check3_scratch(0, db), *d2 = (float *)check3_scratch(1, db), *p1 = (float *)check3_scratch(2, pb), *p2 = (float *)check3_scratch(3, pb);
    if (!(d1 && d2 && p1 && p2)) return;
    for (int rep = 0; rep < 2; ++rep)
        hipLaunchKernelGGL(net_train_h_kernel, dim3(gridb), dim3(kHalfThreads), lds, stream, L, h->params_h, h->params_hb,
                           reinterpret_cast<const uint2 *>(h->d_acts), h->d_dl, n, (float)(1 << k), rep ? d2 : d1, rep ? p2 : p1);
    check3_compare(1, h->d_denc, d1, d2, db, stream);
    check3_compare(1, h->train_partial, p1, p2, pb, stream);
}
static void check3_report()
{
    if (!g_check3.on || !g_check3.dev) return;
    unsigned long long v[16];
    if (hipMemcpy(v, g_check3.dev, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return;
#ifdef WOST_H_NO_REDO
    std::fprintf(stderr, "CHECK3 build: net_forward_h_kernel WITHOUT the recomputed first tile (WOST_H_NO_REDO)\n");
#else
    std::fprintf(stderr, "CHECK3 build: net_forward_h_kernel recomputes a wave's first tile\n");
#endif
    std::fprintf(stderr, "CHECK3 after %llu training steps: forward words differing %llu (odd launch 0/1/2/all: %llu %llu %llu %llu); train kernel words differing %llu (%llu %llu %llu %llu)\n",
                 g_check3.steps, v[0], v[1], v[2], v[3], v[4], v[8], v[9], v[10], v[11], v[12]);
    // where in the launch the forward kernel's differing units lie: a wave takes the tiles blockIdx * waves + wave + k * (256 * waves), k = 0, 1, ...
    const size_t n_log = (size_t)std::min<unsigned long long>(v[0], 65536ull);
    if (n_log) {
        std::vector<uint32_t> idx(n_log);
        if (hipMemcpy(idx.data(), g_check3.log, n_log * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
        const int waves = kHalfFwdThreads / 64;
        std::vector<char> seen;
        size_t hist[16] = {0}, units = 0;
        for (uint32_t w : idx) {
            const size_t unit = (size_t)w / (size_t)g_check3.n_out / 16;
            if (seen.size() <= unit) seen.resize(unit + 1, 0);
            if (seen[unit]) continue;
            seen[unit] = 1;      // (a unit that fails in two different steps is counted once: rare)
            ++units;
            hist[std::min<size_t>(15, unit / 2 / (size_t)(256 * waves))]++;
        }
        std::fprintf(stderr, "CHECK3 forward: %zu distinct units among the first %zu differing words; by the wave's iteration k: ", units, n_log);
        for (int k = 0; k < 16; ++k) std::fprintf(stderr, "%zu ", hist[k]);
        std::fprintf(stderr, "\n");
    }
}
