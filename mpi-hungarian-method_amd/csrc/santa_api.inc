// santa_api.inc — host half of libsanta_hip.so: the context, the design picker,
// one launcher per design and the C-ABI (include/santa_hip.h).
//
// Not a translation unit of its own: santa_hip.hip includes it at its end,
// because the kernels it launches by name are templates in that file's
// anonymous namespace.  Host code lives here so that santa_hip.hip's hash (the
// profile summaries' source_sha16) changes only when device code does.
namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(SH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define HIP_TRY_RC(expr)            \
  do {                              \
    const int rc_ = (expr);         \
    if (rc_ != SH_OK) return rc_;   \
  } while (0)

int pick_k(int n) {
  if (n <= 64) return 1;
  if (n <= 128) return 2;
  if (n <= 256) return 4;
  if (n <= 512) return 8;
  return 16;
}

int64_t miss_units(int n_wish) {
  const float e = (float)(1.0 / (2.0 * n_wish));
  return (int64_t)((double)e * 2147483648.0);
}

// Makes `device` current for the lifetime of the guard and restores the
// caller's device afterwards: every context entry point runs on the context's
// device (allocations, kernel attributes, launches) whatever is current.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) (void)hipSetDevice(device);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// A workgroup's LDS on gfx950, and the dynamic LDS a kernel may ask for before
// its hipFuncAttributeMaxDynamicSharedMemorySize has been raised.
constexpr size_t LDS_MAX = 160 * 1024;
constexpr size_t LDS_NO_ATTR = 64 * 1024;

// Dynamic-LDS attribute already raised for a kernel, per device (attributes
// are per device; a process may drive several).
constexpr int MAX_DEVICES = 64;
struct AttrCache {
  size_t bytes[MAX_DEVICES] = {};
  bool need(int dev, size_t want) const { return dev < 0 || dev >= MAX_DEVICES || bytes[dev] < want; }
  void set(int dev, size_t b) {
    if (dev >= 0 && dev < MAX_DEVICES) bytes[dev] = b;
  }
};

}  // namespace

struct sh_ctx {
  int device;
  int nc, ng, nq, n_wish, n_good;
  int64_t E;
  int16_t *d_wish = nullptr;
  uint32_t *d_wish10 = nullptr;  // packed copy for the in-kernel tile builds (santa_sp3_kernel FUSED, fast_tile_build), or null
  int32_t *d_csr_off = nullptr;
  uint32_t *d_csr = nullptr;
  int32_t *d_err = nullptr;
  // sparse-tile kernel: LDS bytes per block (sets blocks per CU) and the
  // double-buffered overflow lists [2 counters | 2 x ovf_cap block ids]
  int sp_budget = 0;
  int32_t *d_ovf = nullptr;
  int ovf_cap = 0;
  // register-tile sparse design: per-block tile records [rec_cap x SP2_REC]
  unsigned char *d_rec = nullptr;
  int rec_cap = 0;
  int ovf_par = 0;
  int ovf_last = -1;     // the list counter the last solve's primary launch appended to; -1: a design without a fallback launch
  int n_cu = 0;          // compute units
  int dt_slots = 0, dt_slots_n = -1;    // cached dt_tile_slots for one n (pick_design asks every round)
  int64_t *h_mail = nullptr;             // host mailbox (sh_publish_delta): coherent, mapped
  int64_t *d_mail = nullptr;             // its device address
};

namespace {
constexpr int SP_DEFAULT_BUDGET = LDS_MAX / 8;  // 8 blocks (waves) per CU

// Hit-list capacity (entries) of the sparse kernel under the LDS budget: what
// is left after the fixed state and the 64 dump dwords; the hit area also has
// to hold the counting-sort scratch (ng x u32), which may exceed the budget.
int sp_capacity(const sh_ctx *ctx) {
  const SpLds L0 = sp_lds_layout(ctx->ng, 0);
  const size_t budget = (size_t)(ctx->sp_budget > 0 ? ctx->sp_budget : SP_DEFAULT_BUDGET);
  const size_t fixed = L0.hits + 2 * 64 * 2;
  if (budget <= fixed) return 0;
  const size_t cap = (budget - fixed) / 2;
  return (int)std::min<size_t>(cap & ~(size_t)7, 65528);
}
}  // namespace

extern "C" {

const char *sh_last_error(void) { return g_err.c_str(); }

int sh_version(void) { return 1; }

int sh_ctx_create(sh_ctx **out, int device, const int16_t *h_wish, int n_wish,
                  const int32_t *h_goodkids, int n_good, int nc, int ng, int nq) {
  if (!out || !h_wish || !h_goodkids) return fail(SH_ERR_ARGS, "null pointer");
  *out = nullptr;
  if (nc <= 0 || ng <= 0 || nq <= 0 || nc > (1 << 30))
    return fail(SH_ERR_ARGS, "need nc, ng, nq > 0");
  if (n_wish <= 0 || n_wish > 127 || n_wish > ng)
    return fail(SH_ERR_ARGS, "n_wish must be in [1, min(127, ng)]");
  if ((size_t)nc * (size_t)n_wish >= ((size_t)1 << 31))
    return fail(SH_ERR_ARGS, "nc * n_wish must be below 2^31 (32-bit wishlist offsets)");
  if (n_good <= 0 || n_good > 32767 || n_good > nc)
    return fail(SH_ERR_ARGS, "n_good must be in [1, min(32767, nc)]");
  if (ng > 8192) return fail(SH_ERR_ARGS, "ng > 8192 unsupported (LDS chain heads)");
  // validate wishlists: in range and distinct per row
  {
    std::vector<uint32_t> seen((size_t)ng, 0xFFFFFFFFu);
    for (int c = 0; c < nc; ++c) {
      const int16_t *row = h_wish + (size_t)c * n_wish;
      for (int r = 0; r < n_wish; ++r) {
        const int g = row[r];
        if (g < 0 || g >= ng) return fail(SH_ERR_ARGS, "wishlist gift id out of range");
        if (seen[g] == (uint32_t)c) return fail(SH_ERR_ARGS, "wishlist row has a repeated gift");
        seen[g] = (uint32_t)c;
      }
    }
  }
  // inverse good-kids CSR: child -> (gift << 16 | rank), gift-major, rank-ascending
  std::vector<int32_t> off((size_t)nc + 1, 0);
  {
    std::vector<int32_t> seen((size_t)nc, -1);
    for (int g = 0; g < ng; ++g)
      for (int k = 0; k < n_good; ++k) {
        const int c = h_goodkids[(size_t)g * n_good + k];
        if (c < 0 || c >= nc) return fail(SH_ERR_ARGS, "good-kids child id out of range");
        if (seen[c] == g) return fail(SH_ERR_ARGS, "good-kids row has a repeated child");
        seen[c] = g;
        off[(size_t)c + 1]++;
      }
  }
  for (int c = 0; c < nc; ++c) off[(size_t)c + 1] += off[c];
  std::vector<uint32_t> ent((size_t)off[nc]);
  {
    std::vector<int32_t> fillp(off.begin(), off.end() - 1);
    for (int g = 0; g < ng; ++g)
      for (int k = 0; k < n_good; ++k) {
        const int c = h_goodkids[(size_t)g * n_good + k];
        ent[(size_t)fillp[c]++] = ((uint32_t)g << 16) | (uint32_t)k;
      }
  }
  // exactness guard for the twin cost decode (see one_hit_residual)
  const int64_t E = miss_units(n_wish);
  {
    const float e = (float)(1.0 / (2.0 * n_wish));
    if ((double)e * 2147483648.0 != (double)E)
      return fail(SH_ERR_ARGS, "miss value not on the 2^-31 grid");
    for (int a = 1; a <= n_wish; ++a) {
      const float s = (float)(-2.0 * a) + e;
      const int64_t units = (int64_t)((double)s * 2147483648.0);
      if (units != (int64_t)(-a) * 4294967296LL + one_hit_residual(a, E))
        return fail(SH_ERR_ARGS, "twin cost decode mismatch");
    }
    // the 4-wave twins kernel's tile entries (twin_entry) decode to the same costs
    if (E <= 0 || E >= ((int64_t)1 << 31)) return fail(SH_ERR_ARGS, "miss value out of the entry decode's range");
    const int nw1 = n_wish + 1;
    for (int c1 = 0; c1 <= n_wish; ++c1)
      for (int c2 = 0; c2 <= n_wish; ++c2) {
        const int a1 = c1 ? nw1 - c1 : 0, a2 = c2 ? nw1 - c2 : 0, aa = a1 + a2;
        const int64_t m = (c1 && c2) ? 0 : (c1 || c2) ? one_hit_residual(aa, E) : 2 * E;
        const uint32_t e16 = twin_entry((uint32_t)c1 | ((uint32_t)c2 << 8), nw1, E);
        if (e16 > 0xFFFFu || twin_entry_cost<0>(e16, (uint32_t)E) != (int64_t)(-aa) * 4294967296LL + m)
          return fail(SH_ERR_ARGS, "twin tile entry decode mismatch");
      }
  }
  DeviceGuard dg(device);  // the caller's device is current again on return
  sh_ctx *ctx = new sh_ctx();
  ctx->device = device;
  ctx->nc = nc; ctx->ng = ng; ctx->nq = nq; ctx->n_wish = n_wish; ctx->n_good = n_good;
  ctx->E = E;
  auto cleanup = [&](int rc) { sh_ctx_destroy(ctx); return rc; };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return cleanup(fail(SH_ERR_HIP, hipGetErrorString(e)));
  const size_t wb = (size_t)nc * n_wish * sizeof(int16_t);
  if ((e = hipMalloc(&ctx->d_wish, wb + 16)) != hipSuccess ||
      (e = hipMalloc(&ctx->d_csr_off, off.size() * 4)) != hipSuccess ||
      (e = hipMalloc(&ctx->d_csr, std::max<size_t>(ent.size(), 1) * 4)) != hipSuccess ||
      (e = hipMalloc(&ctx->d_err, 16)) != hipSuccess)
    return cleanup(fail(SH_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)));
  if ((e = hipMemcpy(ctx->d_wish, h_wish, wb, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(ctx->d_csr_off, off.data(), off.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
      (ent.size() && (e = hipMemcpy(ctx->d_csr, ent.data(), ent.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) ||
      (e = hipMemset(ctx->d_err, 0, 16)) != hipSuccess)
    return cleanup(fail(SH_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e)));
  // the tile build's packed wishlist: gift r of a row at bits 10 r .. 10 r + 9
  // of its 32-dword line (one 128-byte line per row instead of 200 bytes over
  // two or three)
  if (n_wish % 4 == 0 && n_wish <= 102 && ng <= 1024) {
    std::vector<uint32_t> pk((size_t)nc * 32, 0u);
    for (int c = 0; c < nc; ++c) {
      const int16_t *row = h_wish + (size_t)c * n_wish;
      uint32_t *dst = pk.data() + (size_t)c * 32;
      for (int r = 0; r < n_wish; ++r) {
        const uint32_t g = (uint32_t)row[r], bit = 10u * (uint32_t)r, sh = bit & 31u;
        dst[bit >> 5] |= g << sh;
        if (sh > 22u) dst[(bit >> 5) + 1] |= g >> (32u - sh);
      }
    }
    if ((e = hipMalloc(&ctx->d_wish10, pk.size() * 4)) != hipSuccess ||
        (e = hipMemcpy(ctx->d_wish10, pk.data(), pk.size() * 4, hipMemcpyHostToDevice)) != hipSuccess)
      return cleanup(fail(SH_ERR_HIP, std::string("packed wishlist: ") + hipGetErrorString(e)));
  }
  if ((e = hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess)
    return cleanup(fail(SH_ERR_HIP, hipGetErrorString(e)));
  if ((e = hipHostMalloc((void **)&ctx->h_mail, 8 * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent)) !=
          hipSuccess ||
      (e = hipHostGetDevicePointer((void **)&ctx->d_mail, ctx->h_mail, 0)) != hipSuccess)
    return cleanup(fail(SH_ERR_HIP, std::string("mailbox: ") + hipGetErrorString(e)));
  for (int q = 0; q < 8; ++q) ctx->h_mail[q] = 0;
  *out = ctx;
  return SH_OK;
}

void sh_ctx_destroy(sh_ctx *ctx) {
  if (!ctx) return;
  DeviceGuard dg(ctx->device);
  if (ctx->d_wish) (void)hipFree(ctx->d_wish);
  if (ctx->d_wish10) (void)hipFree(ctx->d_wish10);
  if (ctx->d_csr_off) (void)hipFree(ctx->d_csr_off);
  if (ctx->d_csr) (void)hipFree(ctx->d_csr);
  if (ctx->d_err) (void)hipFree(ctx->d_err);
  if (ctx->d_ovf) (void)hipFree(ctx->d_ovf);
  if (ctx->d_rec) (void)hipFree(ctx->d_rec);
  if (ctx->h_mail) (void)hipHostFree(ctx->h_mail);
  delete ctx;
}

int sh_ctx_set_sparse_budget(sh_ctx *ctx, int bytes) {
  if (!ctx) return fail(SH_ERR_ARGS, "null ctx");
  if (bytes < 0 || (size_t)bytes > LDS_MAX) return fail(SH_ERR_ARGS, "budget must be in [0, 160 KiB]");
  ctx->sp_budget = bytes;
  return sp_capacity(ctx);
}

int sh_ctx_error_flags(sh_ctx *ctx, void *stream) {
  if (!ctx) return fail(SH_ERR_ARGS, "null ctx");
  DeviceGuard dg(ctx->device);
  int32_t h = 0;
  HIP_TRY(hipMemcpyAsync(&h, ctx->d_err, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(ctx->d_err, 0, 4, (hipStream_t)stream));
  return h;
}

int sh_sample_blocks(uint64_t seed, uint64_t round, int lo, int count, int stride, int n, int B,
                     int32_t *d_rows, void *stream) {
  if (!d_rows || n <= 0 || B < 0 || count <= 0 || stride <= 0)
    return fail(SH_ERR_ARGS, "bad sampler arguments");
  if ((int64_t)n * B > count) return fail(SH_ERR_ARGS, "B * n exceeds the eligible count");
  if (B == 0) return SH_OK;
  const ShFeistel f = sh_feistel_make(seed, round, (uint64_t)count);
  const int total = n * B;
  hipLaunchKernelGGL(sample_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, f,
                     lo, stride, total, d_rows, (const int16_t *)nullptr, (int16_t *)nullptr);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

int sh_sample_blocks_undo(uint64_t seed, uint64_t round, int lo, int count, int stride, int n, int B,
                          int32_t *d_rows, const int16_t *d_types, int16_t *d_undo, void *stream) {
  if (!d_rows || !d_types || !d_undo || n <= 0 || B < 0 || count <= 0 || stride <= 0)
    return fail(SH_ERR_ARGS, "bad sampler arguments");
  if ((int64_t)n * B > count) return fail(SH_ERR_ARGS, "B * n exceeds the eligible count");
  if (B == 0) return SH_OK;
  const ShFeistel f = sh_feistel_make(seed, round, (uint64_t)count);
  const int total = n * B;
  hipLaunchKernelGGL(sample_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, f,
                     lo, stride, total, d_rows, d_types, d_undo);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

}  // extern "C"

namespace {
// Raises Kern's dynamic-LDS attribute to `lds` bytes where a launch or an
// occupancy query of that size needs it: above LDS_NO_ATTR, once per device
// and kernel (each instantiation has its own cache), never lowering it.
template <auto Kern>
int raise_lds(const sh_ctx *ctx, size_t lds) {
  static thread_local AttrCache attr;
  if (lds > LDS_NO_ATTR && attr.need(ctx->device, lds)) {
    HIP_TRY(hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr.set(ctx->device, lds);
  }
  return SH_OK;
}

// Dynamic LDS a launch of Kern may ask for: a workgroup's LDS less the
// kernel's static part (256 bytes in the kernels that call __syncthreads_or;
// the runtime refuses a dynamic size that does not leave room for it).
template <auto Kern>
size_t lds_room() {
  static thread_local size_t room = 0;
  if (!room) {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, (const void *)Kern) != hipSuccess) return LDS_MAX;  // (no device: the launch says so)
    room = fa.sharedSizeBytes < LDS_MAX ? LDS_MAX - fa.sharedSizeBytes : 1;
  }
  return room;
}

// Launches Kern with `lds` bytes of dynamic LDS; above lds_room the launch is
// refused with `too_big`.
template <auto Kern, typename... Args>
int launch_lds(const sh_ctx *ctx, const char *too_big, int grid, int block, size_t lds, hipStream_t s,
               const Args &...args) {
  if (lds > lds_room<Kern>()) return fail(SH_ERR_ARGS, too_big);
  HIP_TRY_RC(raise_lds<Kern>(ctx, lds));
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, s, args...);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// Blocks of Kern the device holds at once (occupancy API x CUs).
template <auto Kern>
int occ_blocks(const sh_ctx *ctx, int threads, size_t lds) {
  int per_cu = 0;
  if (lds > lds_room<Kern>()) return 0;
  (void)raise_lds<Kern>(ctx, lds);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kern, threads, lds) != hipSuccess) return 0;
  return per_cu * ctx->n_cu;
}

// A launch over a block list (the fallback launches) loops over its list: one
// workgroup per CU.
int list_grid(const sh_ctx *ctx, int B) { return std::max(1, std::min(B, ctx->n_cu)); }

template <int K, int MODE, bool TIMED = false>
int launch_santa(const sh_ctx *ctx, const SantaArgs &a, int B, hipStream_t s) {
  return launch_lds<santa_block_kernel<K, MODE, TIMED>>(ctx, "block too large for the LDS tile", B, SANTA_WG,
                                                        santa_lds_layout(a.n, MODE, ctx->ng).total, s, a);
}

template <int MODE, int SV = 0>
int launch_santa_vt(const sh_ctx *ctx, const SantaArgs &a, int B, hipStream_t s) {
  const VtLds L = vt_lds_layout(ctx->ng);
  if (L.total > LDS_NO_ATTR) return fail(SH_ERR_ARGS, "too many gift types for the LDS chain heads");
  if ((SV == 0) != (a.blist != nullptr)) return fail(SH_ERR_ARGS, "santa_vt_kernel<0, 0> is the fallback launch only");
  hipLaunchKernelGGL((santa_vt_kernel<MODE, SV>), dim3(a.blist ? list_grid(ctx, B) : B), dim3(VT_WG), L.total, s, a);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// LIST: the launch over santa_lb_kernel's block list (launch_big_list).
template <int MODE, int NW, int K, int FB, bool LIST = false>
int launch_big_cfg(const sh_ctx *ctx, const SantaArgs &a, int B, hipStream_t s) {
  if (a.n > NW * WAVE * K) return fail(SH_ERR_ARGS, "large-block config covers fewer columns than n");
  return launch_lds<santa_big_kernel<MODE, NW, K, FB, LIST>>(ctx, "block too large for LDS", LIST ? list_grid(ctx, B) : B,
                                                             NW * WAVE, big_lds_layout(a.n, MODE, ctx->ng, NW, K).total,
                                                             s, a);
}

// The fallback launch of santa_lb_kernel (singles): a workgroup per CU loops
// over the listed blocks, in with_big_cfg's full-round configuration for
// n <= LB_MAX_N (fewer waves per block: the loop's registers stay out of
// scratch), spelled out so that only these list instantiations exist.
int launch_big_list(const sh_ctx *ctx, const SantaArgs &a, int B, hipStream_t s) {
  if (a.n <= 512) return launch_big_cfg<0, 2, 4, 10, true>(ctx, a, B, s);
  if (a.n <= 1024) return launch_big_cfg<0, 4, 4, 10, true>(ctx, a, B, s);
  return launch_big_cfg<0, 8, 4, 12, true>(ctx, a, B, s);
}

template <int NW_, int K_, int FB_>
struct BigCfg {
  static constexpr int NW = NW_, K = K_, FB = FB_;
};

// The santa_big_kernel configuration of a launch of B blocks of n rows, handed
// to f as a BigCfg<NW, K, FB> tag: one picker for the launch and for its
// occupancy (sh_resident_blocks), so the two cannot drift.
// A full round (at least one block per CU: 477 blocks at n = 2000) runs
// four columns per thread, so ceil(n / 256) waves per block -- fewer waves
// per SIMD competing for issue between each block's barriers than 16: n =
// 2000 round 0 113 -> 78 ms (8 waves; 4 waves x 8 columns: 93 ms), n = 1024
// 101 -> 30 ms and n = 600 76 -> 21 ms (4 waves); the row rebuild takes one
// thread per wish of a unit, (MODE + 1) * n_wish <= NW * 64.  A few blocks
// (twins at 3000 pairs: 6 per round, triplets) keep the wider blocks (a
// lone n = 2000 block: 52 ms at 16 waves, 55 at 8).
// (profiles/r02c_big_rowbuild_ab.jsonl, profiles/r02c_big_nw_ab.jsonl)
template <int MODE, typename F>
int with_big_cfg(const sh_ctx *ctx, int n, int B, F &&f) {
  const bool many = B >= ctx->n_cu;
  if constexpr (MODE == 0) {
    if (many && n <= 512) return f(BigCfg<2, 4, 10>{});
  }
  if constexpr (MODE <= 1) {
    if (many && n > 512 && n <= 1024) return f(BigCfg<4, 4, 10>{});
  }
  if (n <= 512) return f(BigCfg<8, 1, 10>{});
  if (n <= 1024) return f(BigCfg<16, 1, 10>{});
  if (n <= 2048) return many ? f(BigCfg<8, 4, 12>{}) : f(BigCfg<16, 2, 12>{});
  if (n <= 3072) return f(BigCfg<16, 3, 12>{});
  return f(BigCfg<16, 4, 12>{});
}

// The overflow lists of the designs with a fallback launch (block ids, two
// counters that alternate between calls).
int ensure_ovf(sh_ctx *ctx, int B, hipStream_t s) {
  if (ctx->ovf_cap < B) {
    if (ctx->d_ovf) HIP_TRY(hipFree(ctx->d_ovf));
    ctx->d_ovf = nullptr;
    ctx->ovf_cap = 0;
    const int capB = std::max(B, 4096);
    HIP_TRY(hipMalloc(&ctx->d_ovf, (2 + 2 * (size_t)capB) * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(ctx->d_ovf, 0, 2 * sizeof(int32_t), s));
    ctx->ovf_cap = capB;
    ctx->ovf_par = 0;
  }
  return SH_OK;
}

// The designs with a fallback launch: `primary` appends the blocks it leaves
// to an overflow list and `fallback` (launch_santa_vt<0, 0> or
// launch_big_list) walks that list.  All of them share the context's two list
// counters, which alternate between calls: the fallback launch of call k
// resets the counter that call k + 1 appends to.
template <typename P>
int with_fallback(sh_ctx *ctx, SantaArgs a, int B, hipStream_t s, P &&primary,
                  int (*fallback)(const sh_ctx *, const SantaArgs &, int, hipStream_t)) {
  HIP_TRY_RC(ensure_ovf(ctx, B, s));
  const int p = ctx->ovf_par;
  a.ovf_cnt = ctx->d_ovf + p;
  a.ovf_list = ctx->d_ovf + 2 + (size_t)p * ctx->ovf_cap;
  a.blist = nullptr;
  int rc = primary(a);
  if (rc == SH_OK) {
    SantaArgs f = a;
    f.blist = a.ovf_list;
    f.bcount = a.ovf_cnt;
    f.ovf_reset = ctx->d_ovf + (p ^ 1);
    f.undo = nullptr;
    f.nx_rows = nullptr;
    rc = fallback(ctx, f, B, s);
  }
  if (rc) {
    // the primary launch may have appended to counter p: clear it so that a
    // later call's fallback never walks these stale block ids
    (void)hipMemsetAsync(ctx->d_ovf + p, 0, sizeof(int32_t), s);
    return rc;
  }
  ctx->ovf_par = p ^ 1;
  ctx->ovf_last = p;  // (counter p keeps this call's count until the next call's fallback launch resets it)
  return SH_OK;
}

// santa_lb_kernel's configuration for n (NW * 64 * K >= n columns; the word's
// table field holds 2 NW + 2 <= 63 tables)
template <typename F>
int with_lb_cfg(int n, F &&f) {
  if (n <= 512) return f(BigCfg<2, 4, 0>{});
  if (n <= 1024) return f(BigCfg<4, 4, 0>{});
  return f(BigCfg<8, 4, 0>{});
}

bool lb_lds_fits(const sh_ctx *ctx, int n) {
  return with_lb_cfg(n, [&](auto c) -> bool {
    using C = decltype(c);
    return lb_lds_layout(n, ctx->ng, C::NW, C::K).total <= lds_room<santa_lb_kernel<C::NW, C::K>>();
  });
}

// singles blocks the staged-row lattice kernel takes: 256 < n <= 2048 whose
// LDS fits (the tables hold ng int16 entries each), child ids below 2^20 (a
// column's row and child share one 31-bit register)
bool lb_eligible(const sh_ctx *ctx, int n, unsigned flags) {
  return n > 256 && n <= LB_MAX_N && ctx->nc <= (1 << 20) && !(flags & SH_FLAG_BIG_ROWS) &&
         lb_lds_fits(ctx, n);
}

// santa_lb_kernel + santa_big_kernel over the blocks it left (out of its
// lattice range; every block under SH_FLAG_TEST_RANGE / SH_FLAG_EXACT_ARGMIN).
int launch_santa_lb(sh_ctx *ctx, const SantaArgs &args, int B, hipStream_t s) {
  return with_fallback(ctx, args, B, s, [&](const SantaArgs &a) {
    return with_lb_cfg(a.n, [&](auto c) -> int {
      using C = decltype(c);
      static_assert(2 * C::NW + 2 <= 63, "the step word's table field");
      // (the slot sort's scratch: NCOL int16 slot entries in u's n int32)
      if (C::NW * WAVE * C::K > 2 * a.n) return fail(SH_ERR_ARGS, "staged-row kernel: n too small for its config");
      const char *too_big = "staged-row kernel: LDS above 160 KiB";
      const size_t lds = lb_lds_layout(a.n, ctx->ng, C::NW, C::K).total;
      return (a.flags & SH_FLAG_TIMING)
                 ? launch_lds<santa_lb_kernel<C::NW, C::K, true>>(ctx, too_big, B, C::NW * WAVE, lds, s, a)
                 : launch_lds<santa_lb_kernel<C::NW, C::K>>(ctx, too_big, B, C::NW * WAVE, lds, s, a);
    });
  }, launch_big_list);
}

template <int MODE>
int launch_santa_big(const sh_ctx *ctx, const SantaArgs &a, int B, hipStream_t s) {
  return with_big_cfg<MODE>(ctx, a.n, B, [&](auto c) {
    using C = decltype(c);
    return launch_big_cfg<MODE, C::NW, C::K, C::FB>(ctx, a, B, s);
  });
}

// Register-tile 4-wave kernel in scaled units + the windowed-key launch over
// the blocks it left (out of range; every block under the exact-argmin and
// range test flags).
int launch_santa_vt_sc(sh_ctx *ctx, const SantaArgs &args, int B, hipStream_t s) {
  return with_fallback(ctx, args, B, s, [&](const SantaArgs &a) { return launch_santa_vt<0, 1>(ctx, a, B, s); },
                       launch_santa_vt<0, 0>);
}

// Dense-tile one-wave kernel + the windowed-key launch over the blocks it
// left (out of range; every block under the exact-argmin and range test
// flags).
int launch_santa_dt(sh_ctx *ctx, const SantaArgs &args, int B, hipStream_t s) {
  // the tile holds rank codes (rank + 1) in uint8 with 255 the miss, and a
  // miss's key-unit cost (n_wish + 1) << 20 | 2^11 must stay below 255 << 20:
  // the same guard as the default dispatch, here also for the forced
  // SH_FLAG_DT_TILE (sh_ctx_create caps n_wish at 127 today, well inside it)
  if (ctx->n_wish > 253) return fail(SH_ERR_ARGS, "dense tile: n_wish > 253 does not fit the uint8 rank codes");
  const size_t lds = dt_lds_layout(args.n, ctx->ng).total;
  const char *too_big = "dense tile: too many gift types for LDS";
  if (lds > lds_room<santa_dt_kernel<false>>()) return fail(SH_ERR_ARGS, too_big);  // (before the overflow lists are made)
  return with_fallback(ctx, args, B, s, [&](const SantaArgs &a) {
    return (a.flags & SH_FLAG_TIMING) ? launch_lds<santa_dt_kernel<true>>(ctx, too_big, B, SANTA_WG, lds, s, a)
                                      : launch_lds<santa_dt_kernel<false>>(ctx, too_big, B, SANTA_WG, lds, s, a);
  }, launch_santa_vt<0, 0>);
}

// Sparse-tile kernel + the fallback launch for blocks whose hit lists did not
// fit.
int launch_santa_sp(sh_ctx *ctx, SantaArgs args, int B, hipStream_t s, bool tile2) {
  const int cap = sp_capacity(ctx);
  const size_t lds = tile2 ? tile_lds_layout(ctx->ng).total : sp_lds_layout(ctx->ng, cap).total;
  if (lds > LDS_NO_ATTR) return fail(SH_ERR_ARGS, "sparse-tile LDS budget above 64 KiB");
  const bool fused = tile2 && ctx->d_wish10;  // (in-kernel build: packed wishlists only)
  if (tile2 && !fused && ctx->rec_cap < B) {  // per-block tile records (HBM)
    if (ctx->d_rec) HIP_TRY(hipFree(ctx->d_rec));
    ctx->d_rec = nullptr;
    ctx->rec_cap = 0;
    const int capB = std::max(B, 4096);
    HIP_TRY(hipMalloc(&ctx->d_rec, (size_t)capB * SP2_REC));
    ctx->rec_cap = capB;
  }
  args.cap = cap;
  if (tile2) {
    // overflow capacity per block; a sparse budget set for tests lowers it
    // (budget / 16 entries) so that some or all blocks take the fallback
    const int ocap = fused ? SP4_OVF_CAP : SP2_OVF_CAP;
    args.cap = ctx->sp_budget > 0 ? std::min(ocap, ctx->sp_budget / 16) : ocap;
  }
  const bool vec = ctx->n_wish % 4 == 0;
  return with_fallback(ctx, args, B, s, [&](const SantaArgs &a) -> int {
    if (fused) {  // one kernel: each wave builds its block's tile, then solves it
      if (a.flags & SH_FLAG_TIMING)
        hipLaunchKernelGGL((santa_sp3_kernel<true, true>), dim3(B), dim3(WAVE), 0, s, a, nullptr);
      else
        hipLaunchKernelGGL((santa_sp3_kernel<false, true>), dim3(B), dim3(WAVE), 0, s, a, nullptr);
    } else if (tile2) {
      if (vec)
        hipLaunchKernelGGL(santa_tile_kernel<1>, dim3(B), dim3(TILE_NW * WAVE), lds, s, a, ctx->d_rec);
      else
        hipLaunchKernelGGL(santa_tile_kernel<0>, dim3(B), dim3(TILE_NW * WAVE), lds, s, a, ctx->d_rec);
      HIP_TRY(hipGetLastError());
      if (a.flags & SH_FLAG_TIMING)
        hipLaunchKernelGGL((santa_sp3_kernel<true, false>), dim3(B), dim3(WAVE), 0, s, a,
                           (const unsigned char *)ctx->d_rec);
      else
        hipLaunchKernelGGL((santa_sp3_kernel<false, false>), dim3(B), dim3(WAVE), 0, s, a,
                           (const unsigned char *)ctx->d_rec);
    } else if (vec)
      hipLaunchKernelGGL(santa_sp_kernel<true>, dim3(B), dim3(WAVE), lds, s, a);
    else
      hipLaunchKernelGGL(santa_sp_kernel<false>, dim3(B), dim3(WAVE), lds, s, a);
    HIP_TRY(hipGetLastError());
    return SH_OK;
  }, launch_santa_vt<0, 0>);
}
}  // namespace

namespace {
// Flags of designs that left the library: SH_FLAG_SW_TILE (the one-wave
// register-tile kernel, round 3), SH_FLAG_SP2 (santa_sp2_kernel, round 2's
// 64-bit-key one-wave kernel, round 4).
int refuse_retired(unsigned flags) {
  if (flags & SH_FLAG_SW_TILE)
    return fail(SH_ERR_ARGS, "SH_FLAG_SW_TILE: the one-wave register-tile design is retired");
  if (flags & SH_FLAG_SP2)
    return fail(SH_ERR_ARGS, "SH_FLAG_SP2: the 64-bit-key one-wave design (santa_sp2_kernel) is retired");
  return SH_OK;
}

// The mode, n and B of a solve or of a question about one.
int check_mode_n_B(int mode, int n, int B) {
  if (mode != SH_MODE_SINGLE && mode != SH_MODE_TWINS && mode != SH_MODE_TRIPLETS)
    return fail(SH_ERR_ARGS, "bad mode");
  if (n <= 0 || n > SH_MAX_N_SANTA) return fail(SH_ERR_ARGS, "n must be in [1, 4096]");
  if (B < 0) return fail(SH_ERR_ARGS, "B < 0");
  return SH_OK;
}

// Dense-tile one-wave blocks (singles) the device holds at once for this n;
// cached for the last n, since pick_design asks every round.
int dt_tile_slots(sh_ctx *ctx, int n) {
  if (ctx->dt_slots_n != n) {
    ctx->dt_slots = occ_blocks<santa_dt_kernel<false>>(ctx, SANTA_WG, dt_lds_layout(n, ctx->ng).total);
    ctx->dt_slots_n = n;
  }
  return ctx->dt_slots;
}

int pick_design(sh_ctx *ctx, int mode, int n, int B, unsigned flags) {
  // triplets (a few blocks per round: 1667 units) rebuild each row from the wishlists
  if (n > 256 && mode == SH_MODE_SINGLE && lb_eligible(ctx, n, flags)) return SH_DESIGN_LARGE_LB;
  if (n > 256 || mode == SH_MODE_TRIPLETS) return SH_DESIGN_LARGE;
  // twins keep the LDS tile: their 128-dword register column does not stay
  // in VGPRs (the compiler moves it to scratch), and a round has 78 blocks
  // (a one-wave dense-tile twins kernel with 64-bit keys was built in round 4
  // and measured 36 % slower than this 4-wave one: profiles/r04_twins_dt.jsonl)
  // (the code-pair tile, 2 n r16(n) bytes, and the ng chain heads share the
  // workgroup's LDS: where they do not fit lds_room -- n = 256 from ng = 6569
  // -- the row-rebuild kernel takes the block, as it does for n > 256)
  if (mode == SH_MODE_TWINS)
    return santa_lds_layout(n, 1, ctx->ng).total <= lds_room<santa_block_kernel<1, 1>>() ? SH_DESIGN_TWINS
                                                                                             : SH_DESIGN_LARGE;
  if (flags & SH_FLAG_LDS_TILE) return SH_DESIGN_LDS_TILE;
  if (flags & SH_FLAG_DT_TILE) return SH_DESIGN_DT_TILE;
  // (SH_FLAG_SW_TILE, the retired one-wave register-tile kernel, is refused
  // by the entry points)
  // the sparse kernel packs child ids (< 2^20) and gift types (< 1023) in one
  // dword during its build; other instances take the register-tile kernel
  if ((flags & SH_FLAG_VT_TILE) || ctx->nc > (1 << 20) || ctx->ng > 1022) return SH_DESIGN_VT_TILE;
  // the register-tile sparse kernel keeps the wish value in 7 bits with one
  // code reserved (n_wish <= 126); the LDS-list kernel takes the rest
  const int sparse = (ctx->n_wish > 126 || (flags & SH_FLAG_SP1)) ? SH_DESIGN_SPARSE : SH_DESIGN_SPARSE3;
  if (flags & (SH_FLAG_SP_TILE | SH_FLAG_SP1)) return sparse;
  // few blocks (at most one resident wave of dense-tile blocks, two per CU):
  // every block starts at once and the launch takes one block's latency,
  // which the one-wave dense-tile kernel has lowest (round 4, MI355X, one
  // GPU's shard of a round at 8 GPUs, 466 blocks: 1.13 ms at round 0 against
  // 1.36 for the 4-wave LDS tile and 1.45 for the sparse kernel, 0.49 / 0.52
  // / 0.65 ms at round 10; profiles/r04_shard_dt.jsonl).  Beyond it the
  // sparse kernel: at 933 blocks (the shard at 4 GPUs) 1.52 ms against 1.60
  // for the 4-wave register tile and 1.76 for two waves of dense-tile blocks.
  if (ctx->n_wish <= 253 && B <= dt_tile_slots(ctx, n)) return SH_DESIGN_DT_TILE;
  return sparse;
}

template <int MODE>
int big_resident(const sh_ctx *ctx, int n, int B) {  // the configuration launch_santa_big picks
  return with_big_cfg<MODE>(ctx, n, B, [&](auto c) {
    using C = decltype(c);
    return occ_blocks<santa_big_kernel<MODE, C::NW, C::K, C::FB>>(ctx, C::NW * WAVE,
                                                                  big_lds_layout(n, MODE, ctx->ng, C::NW, C::K).total);
  });
}

int resident_blocks(sh_ctx *ctx, int design, int mode, int n, int B) {
  switch (design) {
    case SH_DESIGN_LARGE:
      return mode == SH_MODE_SINGLE ? big_resident<0>(ctx, n, B)
             : mode == SH_MODE_TWINS ? big_resident<1>(ctx, n, B) : big_resident<2>(ctx, n, B);
    case SH_DESIGN_LARGE_LB:
      return with_lb_cfg(n, [&](auto c) {
        using C = decltype(c);
        return occ_blocks<santa_lb_kernel<C::NW, C::K>>(ctx, C::NW * WAVE, lb_lds_layout(n, ctx->ng, C::NW, C::K).total);
      });
    case SH_DESIGN_TWINS:
      return occ_blocks<santa_block_kernel<1, 1>>(ctx, SANTA_WG, santa_lds_layout(n, 1, ctx->ng).total);
    case SH_DESIGN_LDS_TILE:
      return occ_blocks<santa_block_kernel<1, 0>>(ctx, SANTA_WG, santa_lds_layout(n, 0, ctx->ng).total);
    case SH_DESIGN_DT_TILE: return dt_tile_slots(ctx, n);
    case SH_DESIGN_VT_TILE: return occ_blocks<santa_vt_kernel<0, 1>>(ctx, VT_WG, vt_lds_layout(ctx->ng).total);
    case SH_DESIGN_SPARSE3:
      return ctx->d_wish10 ? occ_blocks<santa_sp3_kernel<false, true>>(ctx, WAVE, 0)
                           : occ_blocks<santa_sp3_kernel<false, false>>(ctx, WAVE, 0);
    default:
      return occ_blocks<santa_sp_kernel<true>>(ctx, WAVE, sp_lds_layout(ctx->ng, sp_capacity(ctx)).total);
  }
}
}  // namespace

extern "C" {

int sh_solve_blocks(sh_ctx *ctx, int mode, const int32_t *d_rows, int n, int B, int16_t *d_types,
                    int32_t *d_col, int64_t *d_cost, int64_t *d_delta, int64_t *d_steps,
                    unsigned flags, void *stream) {
  return sh_solve_round(ctx, mode, d_rows, n, B, d_types, d_col, d_cost, d_delta, d_steps, nullptr, flags, stream);
}

int sh_solve_round(sh_ctx *ctx, int mode, const int32_t *d_rows, int n, int B, int16_t *d_types,
                   int32_t *d_col, int64_t *d_cost, int64_t *d_delta, int64_t *d_steps, const sh_round_ext *ext,
                   unsigned flags, void *stream) {
  if (!ctx || (!d_rows && B > 0) || !d_types) return fail(SH_ERR_ARGS, "null pointer");
  const bool sample = ext && ext->next_rows && ext->next_B > 0;
  if (sample && (ext->next_count <= 0 || ext->next_stride <= 0 || (int64_t)n * ext->next_B > ext->next_count))
    return fail(SH_ERR_ARGS, "bad next-round sampler arguments");
  const bool publish = ext && ext->publish;
  if (publish && (!d_delta || ext->publish_slot < 0 || ext->publish_slot > 1))
    return fail(SH_ERR_ARGS, "bad mailbox arguments");
  HIP_TRY_RC(check_mode_n_B(mode, n, B));
  if ((int64_t)n * (mode + 1) > ctx->nc) return fail(SH_ERR_ARGS, "block larger than the instance");
  {  // the next round's rows and the undo record are written while other
     // workgroups still read this round's rows and types: no overlap allowed
    auto overlap = [](const void *p, size_t np, const void *q, size_t nq) {
      const uintptr_t a0 = (uintptr_t)p, b0 = (uintptr_t)q;
      return p && q && np && nq && a0 < b0 + nq && b0 < a0 + np;
    };
    const size_t rows_b = (size_t)n * (size_t)B * 4, types_b = (size_t)ctx->nc * 2;
    if (sample && (overlap(ext->next_rows, (size_t)n * ext->next_B * 4, d_rows, rows_b) ||
                   overlap(ext->next_rows, (size_t)n * ext->next_B * 4, d_types, types_b)))
      return fail(SH_ERR_ARGS, "next_rows overlaps d_rows or d_types");
    if (ext && ext->d_undo && (overlap(ext->d_undo, (size_t)n * B * 2, d_rows, rows_b) ||
                               overlap(ext->d_undo, (size_t)n * B * 2, d_types, types_b) ||
                               (sample && overlap(ext->d_undo, (size_t)n * B * 2, ext->next_rows,
                                                  (size_t)n * ext->next_B * 4))))
      return fail(SH_ERR_ARGS, "d_undo overlaps d_rows, d_types or next_rows");
  }
  HIP_TRY_RC(refuse_retired(flags));
  DeviceGuard dg(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  ctx->ovf_last = -1;
  if (B == 0) {
    if (publish) HIP_TRY_RC(sh_publish_delta(ctx, d_delta, ext->publish_slot, ext->publish_seq, stream));
    return SH_OK;
  }
  SantaArgs a;
  a.rows = d_rows; a.types = d_types; a.col = d_col; a.cost = d_cost; a.delta = d_delta;
  a.steps = d_steps; a.wish = ctx->d_wish; a.wish10 = ctx->d_wish10; a.csr_off = ctx->d_csr_off; a.csr = ctx->d_csr;
  a.err = ctx->d_err; a.E = ctx->E; a.n = n; a.nc = ctx->nc; a.ng = ctx->ng;
  a.n_wish = ctx->n_wish; a.n_good = ctx->n_good; a.flags = flags;
  a.cap = 0; a.ovf_cnt = nullptr; a.ovf_list = nullptr;
  a.blist = nullptr; a.bcount = nullptr; a.ovf_reset = nullptr;
  a.undo = ext ? ext->d_undo : nullptr;
  a.nx_rows = nullptr;
  a.nx_lo = a.nx_stride = a.nx_total = 0;
  a.nx_f = ShFeistel{};
  if (sample) {
    a.nx_rows = ext->next_rows;
    a.nx_f = sh_feistel_make(ext->next_seed, ext->next_round, (uint64_t)ext->next_count);
    a.nx_lo = ext->next_lo;
    a.nx_stride = ext->next_stride;
    a.nx_total = n * ext->next_B;
  }
  a.pub_mail = nullptr;
  a.pub_seq = 0;
  a.pub_cnt = ctx->d_err + 2;
  const int design = pick_design(ctx, mode, n, B, flags);
  // designs whose last launch is the fallback santa_vt_kernel<0, 0>: its last
  // workgroup publishes (one launch fewer between two rounds); the others
  // enqueue publish_kernel after their launches
  const bool fold = design == SH_DESIGN_SPARSE || design == SH_DESIGN_SPARSE3 || design == SH_DESIGN_DT_TILE ||
                    design == SH_DESIGN_VT_TILE;
  if (publish && fold) {
    a.pub_mail = ctx->d_mail + 4 * ext->publish_slot;
    a.pub_seq = ext->publish_seq;
  }
  int rc;
  switch (design) {
    case SH_DESIGN_LARGE:
      rc = mode == SH_MODE_SINGLE ? launch_santa_big<0>(ctx, a, B, s)
           : mode == SH_MODE_TWINS ? launch_santa_big<1>(ctx, a, B, s)
                                   : launch_santa_big<2>(ctx, a, B, s);
      break;
    case SH_DESIGN_LARGE_LB: rc = launch_santa_lb(ctx, a, B, s); break;
    case SH_DESIGN_TWINS:
      rc = (flags & SH_FLAG_TIMING) ? launch_santa<1, 1, true>(ctx, a, B, s) : launch_santa<1, 1>(ctx, a, B, s);
      break;
    case SH_DESIGN_LDS_TILE:
      rc = (flags & SH_FLAG_TIMING) ? launch_santa<1, 0, true>(ctx, a, B, s) : launch_santa<1, 0>(ctx, a, B, s);
      break;
    case SH_DESIGN_VT_TILE: rc = launch_santa_vt_sc(ctx, a, B, s); break;
    case SH_DESIGN_DT_TILE: rc = launch_santa_dt(ctx, a, B, s); break;
    case SH_DESIGN_SPARSE3: rc = launch_santa_sp(ctx, a, B, s, true); break;
    default: rc = launch_santa_sp(ctx, a, B, s, false); break;
  }
  if (rc == SH_OK && publish && !fold) rc = sh_publish_delta(ctx, d_delta, ext->publish_slot, ext->publish_seq, stream);
  return rc;
}

int sh_solve_design(sh_ctx *ctx, int mode, int n, int B, unsigned flags) {
  if (!ctx) return fail(SH_ERR_ARGS, "null ctx");
  HIP_TRY_RC(check_mode_n_B(mode, n, B));
  HIP_TRY_RC(refuse_retired(flags));
  DeviceGuard dg(ctx->device);
  return pick_design(ctx, mode, n, B, flags);
}

int sh_resident_blocks(sh_ctx *ctx, int mode, int n, int B, unsigned flags) {
  if (!ctx) return fail(SH_ERR_ARGS, "null ctx");
  HIP_TRY_RC(check_mode_n_B(mode, n, B));
  HIP_TRY_RC(refuse_retired(flags));
  DeviceGuard dg(ctx->device);
  return resident_blocks(ctx, pick_design(ctx, mode, n, B, flags), mode, n, B);
}

int sh_ctx_fallback_steps(sh_ctx *ctx, void *stream) {
  if (!ctx) return fail(SH_ERR_ARGS, "null ctx");
  DeviceGuard dg(ctx->device);
  int32_t h = 0;
  HIP_TRY(hipMemcpyAsync(&h, ctx->d_err + 1, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(ctx->d_err + 1, 0, 4, (hipStream_t)stream));
  return h;
}

int sh_ctx_fallback_blocks(sh_ctx *ctx, void *stream) {
  if (!ctx) return fail(SH_ERR_ARGS, "null ctx");
  if (ctx->ovf_last < 0 || !ctx->d_ovf) return 0;
  DeviceGuard dg(ctx->device);
  int32_t h = 0;
  HIP_TRY(hipMemcpyAsync(&h, ctx->d_ovf + ctx->ovf_last, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return h;
}

int sh_score(sh_ctx *ctx, const int16_t *d_types, int64_t *d_sums, void *stream) {
  if (!ctx || !d_types || !d_sums) return fail(SH_ERR_ARGS, "null pointer");
  DeviceGuard dg(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_sums, 0, 4 * sizeof(int64_t), s));
  ScoreArgs a;
  a.wish = ctx->d_wish; a.csr_off = ctx->d_csr_off; a.csr = ctx->d_csr; a.types = d_types;
  a.sums = d_sums; a.nc = ctx->nc; a.n_wish = ctx->n_wish; a.n_good = ctx->n_good;
  const int twins = (int)ceil(0.04 * ctx->nc / 2.) * 2;
  const int triplets = (int)ceil(0.005 * ctx->nc / 3.) * 3;
  a.n_tri = triplets; a.n_twin = twins;
  const int chunks = (ctx->nc + WAVE - 1) / WAVE;
  const int grid = std::min((chunks + SCORE_WAVES - 1) / SCORE_WAVES, 2048);
  hipLaunchKernelGGL(score_kernel, dim3(grid), dim3(WAVE * SCORE_WAVES), 0, s, a);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

int64_t *sh_ctx_mailbox(sh_ctx *ctx) { return ctx ? ctx->h_mail : nullptr; }

int sh_publish_delta(sh_ctx *ctx, int64_t *d_delta, int slot, int64_t seq, void *stream) {
  if (!ctx || !d_delta || slot < 0 || slot > 1) return fail(SH_ERR_ARGS, "bad mailbox arguments");
  DeviceGuard dg(ctx->device);
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_delta, ctx->d_mail + 4 * slot,
                     seq);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

int sh_pack_types(const int16_t *d_types, const int32_t *d_rows, int count, int16_t *d_out,
                  void *stream) {
  if (count < 0) return fail(SH_ERR_ARGS, "count < 0");
  if (count == 0) return SH_OK;
  hipLaunchKernelGGL(pack_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     d_types, d_rows, count, d_out);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

int sh_unpack_types(int16_t *d_types, const int32_t *d_rows, int count, const int16_t *d_in,
                    int mode, void *stream) {
  if (count < 0) return fail(SH_ERR_ARGS, "count < 0");
  if (mode < SH_MODE_SINGLE || mode > SH_MODE_TRIPLETS) return fail(SH_ERR_ARGS, "bad mode");
  if (count == 0) return SH_OK;
  hipLaunchKernelGGL(unpack_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     d_types, d_rows, count, d_in, mode);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

}  // extern "C"

namespace {
// nr x nc instances (the square entries: nr == nc == n); host-side only.
// cap: SH_MAX_N, or SH_MAX_N_LARGE for the lsap_*_large_ and lsap_solve_csr_ entries.
int check_lsap_args(int nr, int nc, int B, const int32_t *col, int cap) {
  if (nr < 1 || nc > cap)
    return fail(SH_ERR_ARGS, cap == SH_MAX_N ? "sizes must be in [1, 1024]" : "sizes must be in [1, 4096]");
  if (nr > nc) return fail(SH_ERR_ARGS, "nr > nc: transpose tall input (as scipy does) and solve that");
  if (B < 0) return fail(SH_ERR_ARGS, "B < 0");
  if (!col && B > 0) return fail(SH_ERR_ARGS, "null col");
  return SH_OK;
}

// The checks of the lsap_solve_batched_rect_ entries and, with `duals` (u and
// v required), of the lsap_solve_batched_duals_ ones: up to SH_MAX_N columns.
template <typename T>
int check_solve(const void *C, int nr, int nc, int B, const int32_t *col, bool duals, const T *du, const T *dv) {
  if (!C && B > 0) return fail(SH_ERR_ARGS, "null C");
  HIP_TRY_RC(check_lsap_args(nr, nc, B, col, SH_MAX_N));
  if (duals && (!du || !dv) && B > 0) return fail(SH_ERR_ARGS, "null u or v");
  return SH_OK;
}

// Those of the lsap_solve_large_ entries: up to SH_MAX_N_LARGE columns, the
// sizes first, u and v nullable.
template <typename T>
int check_large_solve(const void *C, int nr, int nc, int B, const int32_t *col, const T *du, const T *dv) {
  HIP_TRY_RC(check_lsap_args(nr, nc, B, col, SH_MAX_N_LARGE));
  if (!C && B > 0) return fail(SH_ERR_ARGS, "null C");
  if ((du == nullptr) != (dv == nullptr)) return fail(SH_ERR_ARGS, "u and v: both or neither");
  return SH_OK;
}

// A solve kernel's duals form is the same kernel with `T *du, T *dv` as a
// trailing parameter pack.  f(d...) receives (du, dv) when the caller passed
// them and nothing otherwise, and names its kernel with decltype(d)..., so a
// launch is written once for both forms.  CAN = false: no duals form exists.
template <bool CAN = true, typename T, typename F>
void with_duals(T *du, T *dv, F &&f) {
  if constexpr (CAN) {
    if (du) return f(du, dv);
  }
  f();
}

template <int V>
using int_c = std::integral_constant<int, V>;

// The (NW, K) of a launch beyond SH_MAX_N columns by its column slots, handed
// to f as a BigCfg<NW, K, 12> tag.  Integer costs take with_big_cfg's table for
// a batch that fills the chip: four columns per thread up to 2048 columns on 8
// waves, 16 waves beyond with three columns where they cover the instance (16 x
// 2 at 2000 columns: 5 % faster up to 256 instances, equal at 1024; not taken).
// Float costs stay on 8 waves with more columns per thread: every wave folds
// the NW (value, key, row) slots of a step, and 16 of them cost more than the
// columns spread over them save (2000 columns, 16 x 2 against 8 x 4: 25 %
// slower, 2x at 1024 instances; 3000 columns, 8 x 6 against 16 x 3: 14 - 18 %
// faster; 4096, 8 x 8 against 16 x 4: 3 - 10 %; DESIGN §7,
// profiles/lsap_large.jsonl).
template <typename F>
int with_large_cfg(int nc, F &&f) {
  if (nc <= 2048) return f(BigCfg<8, 4, 12>{});
  if (nc <= 3072) return f(BigCfg<16, 3, 12>{});
  return f(BigCfg<16, 4, 12>{});
}

template <typename F>
int with_large_f64_cfg(int nc, F &&f) {
  if (nc <= 2048) return f(BigCfg<8, 4, 12>{});
  if (nc <= 3072) return f(BigCfg<8, 6, 12>{});
  return f(BigCfg<8, 8, 12>{});
}

// Integer costs: S (int64_t, int32_t) read from C or, with HASH, generated from
// (seed, mod).  The one launch table of lsap_i64_kernel, for every entry; the
// entries' checks (above) come first.  The configuration follows the column
// slots n (a thread owns K of them, as in the square case), the LDS size the
// rows and columns (lsap_i64_lds).  HASH has neither a duals form nor
// instances beyond SH_MAX_N columns.
template <typename S, bool HASH>
int launch_i64(const S *C, uint64_t seed, int64_t mod, int nr, int n, int B, const int32_t *shape, int32_t *col,
               int64_t *cost, int64_t *du, int64_t *dv, unsigned flags, hipStream_t s) {
  if (B == 0) return SH_OK;
  auto go = [&](auto cfg) {
    using C_ = decltype(cfg);
    const size_t lds = lsap_i64_lds(nr, n, C_::NW, C_::FB);
    with_duals<!HASH>(du, dv, [&](auto... d) {
      auto launch = [&](auto rect) {
        hipLaunchKernelGGL((lsap_i64_kernel<C_::NW, C_::K, S, HASH, decltype(rect)::value, C_::FB, decltype(d)...>),
                           dim3(B), dim3(C_::NW * WAVE), lds, s, C, seed, mod, nr, n, shape, col, cost,
                           (int32_t *)nullptr, flags, d...);
      };
      // the square form (RECT = false): the 10-bit key without duals, and no other
      if constexpr (C_::FB == 10 && sizeof...(d) == 0) {
        if (nr == n && !shape) return launch(std::false_type{});
      }
      launch(std::true_type{});
    });
    HIP_TRY(hipGetLastError());
    return SH_OK;
  };
  if constexpr (!HASH) {
    if (n > SH_MAX_N) return with_large_cfg(n, go);
  }
  // a batch that fills the chip many times over runs one wave per instance
  // with several columns per thread (fewer waves per block, more blocks per
  // CU: the large-block kernel's lesson): n <= 128 from 4096 instances
  // (65536 hash-generated: 1.45 -> 2.49 M solves/s), n = 256 from 65536
  // (397 -> 443 k/s; at 4096 it lost 17 %); n = 512 gained nothing
  // (profiles/r02e_lsap_sweep_ab.jsonl)
  if (n <= WAVE) return go(BigCfg<1, 1, 10>{});
  if (B >= 4096 && n <= 128) return go(BigCfg<1, 2, 10>{});
  if (B >= 65536 && n <= 256) return go(BigCfg<1, 4, 10>{});
  if (n <= 256) return go(BigCfg<4, 1, 10>{});
  if (n <= 512) return go(BigCfg<4, 2, 10>{});
  return go(BigCfg<4, 4, 10>{});
}

template <typename S>
int solve_i64(const S *C, int nr, int n, int B, const int32_t *shape, int32_t *col, int64_t *cost, int64_t *du,
              int64_t *dv, unsigned flags, hipStream_t s) {
  return launch_i64<S, false>(C, 0, 1, nr, n, B, shape, col, cost, du, dv, flags, s);
}

// Whether a float batch of B instances with nc columns runs four waves per
// instance by default (measured: DESIGN §7, profiles/lsap_float_ab.jsonl).
// Up to 1024 instances one wave each leaves SIMDs idle and four waves won at
// every nc measured (128: 5-9 %, 256: 17-22 %, 512: 29-36 %, 1024: 38-49 %);
// at 4096 instances one wave each won (nc = 128, 256, 512), and nothing
// between 1024 and 4096 was measured except nc = 256 (2048: four waves, 5 %),
// so those batches keep the kernel they always ran.
bool f64_mw_default(int nc, int B) { return nc > WAVE && B <= 1024; }

int check_f64_flags(unsigned flags, int n) {
  if ((flags & SH_FLAG_F64_MW) && (flags & SH_FLAG_F64_SW))
    return fail(SH_ERR_ARGS, "SH_FLAG_F64_MW and SH_FLAG_F64_SW exclude each other");
  if ((flags & SH_FLAG_F64_SW) && n > SH_MAX_N)
    return fail(SH_ERR_ARGS, "SH_FLAG_F64_SW: no one-wave float kernel above 1024 columns");
  return SH_OK;
}

// A float launch's cost source: the two kernels of a kind of costs and their
// leading arguments.  Dense costs stored as S (double, float, _Float16,
// sh_bf16), or CSR (double, float) after lsap_csr_prep_kernel.
template <typename S>
struct DenseF64 {
  const S *C;
  template <int K, typename... DU>
  void one_wave(int B, size_t lds, hipStream_t s, int nr, int n, const int32_t *shape, int32_t *col, double *cost,
                DU... d) const {
    hipLaunchKernelGGL((lsap_f64_kernel<K, S, DU...>), dim3(B), dim3(WAVE), lds, s, C, nr, n, shape, col, cost, d...);
  }
  template <int NW, int K, int FB, typename... DU>
  void multi_wave(int B, size_t lds, hipStream_t s, int nr, int n, const int32_t *shape, int32_t *col, double *cost,
                  DU... d) const {
    hipLaunchKernelGGL((lsap_f64_mw_kernel<NW, K, S, FB, DU...>), dim3(B), dim3(NW * WAVE), lds, s, C, nr, n, shape,
                       col, cost, d...);
  }
};

template <typename S>
struct CsrF64 {
  const int64_t *indptr;
  const S *data;
  const uint64_t *mask;
  const uint16_t *pre;
  template <int K, typename... DU>
  void one_wave(int B, size_t lds, hipStream_t s, int nr, int n, const int32_t *shape, int32_t *col, double *cost,
                DU... d) const {
    hipLaunchKernelGGL((lsap_csr_kernel<K, S, DU...>), dim3(B), dim3(WAVE), lds, s, indptr, data, mask, pre, nr, n,
                       shape, col, cost, d...);
  }
  template <int NW, int K, int FB, typename... DU>
  void multi_wave(int B, size_t lds, hipStream_t s, int nr, int n, const int32_t *shape, int32_t *col, double *cost,
                  DU... d) const {
    hipLaunchKernelGGL((lsap_csr_mw_kernel<NW, K, S, FB, DU...>), dim3(B), dim3(NW * WAVE), lds, s, indptr, data, mask,
                       pre, nr, n, shape, col, cost, d...);
  }
};

// Floating-point costs, solved in float64: the one launch table of the float
// kernels, for every entry and both sources; the entries' checks (above) come
// first.  One wave per instance (lsap_f64_lds) or, for n > 64, four (1 / 2 / 4
// columns per thread as the integer path's; lsap_f64_mw_lds): the default is
// f64_mw_default, SH_FLAG_F64_MW / SH_FLAG_F64_SW force one.  Beyond SH_MAX_N
// columns with_large_f64_cfg's eight waves.
template <typename Src>
int launch_f64(const Src &src, int nr, int n, int B, const int32_t *shape, int32_t *col, double *cost, double *du,
               double *dv, unsigned flags, hipStream_t s) {
  HIP_TRY_RC(check_f64_flags(flags, n));
  if (B == 0) return SH_OK;
  with_duals(du, dv, [&](auto... d) {
    auto mw = [&](auto cfg) {
      using C_ = decltype(cfg);
      src.template multi_wave<C_::NW, C_::K, C_::FB>(B, lsap_f64_mw_lds(nr, n, C_::NW, C_::FB), s, nr, n, shape,
                                                     col, cost, d...);
      return SH_OK;
    };
    auto sw = [&](auto k) {
      src.template one_wave<decltype(k)::value>(B, lsap_f64_lds(nr), s, nr, n, shape, col, cost, d...);
    };
    if (n > SH_MAX_N) {
      with_large_f64_cfg(n, mw);
    } else if (n > WAVE && !(flags & SH_FLAG_F64_SW) && ((flags & SH_FLAG_F64_MW) || f64_mw_default(n, B))) {
      if (n <= 256) mw(BigCfg<4, 1, 10>{});
      else if (n <= 512) mw(BigCfg<4, 2, 10>{});
      else mw(BigCfg<4, 4, 10>{});
    } else {
      switch (pick_k(n)) {
        case 1: sw(int_c<1>{}); break;
        case 2: sw(int_c<2>{}); break;
        case 4: sw(int_c<4>{}); break;
        case 8: sw(int_c<8>{}); break;
        default: sw(int_c<16>{}); break;
      }
    }
  });
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

template <typename S>
int solve_f64(const S *C, int nr, int n, int B, const int32_t *shape, int32_t *col, double *cost, double *du,
              double *dv, unsigned flags, hipStream_t s) {
  return launch_f64(DenseF64<S>{C}, nr, n, B, shape, col, cost, du, dv, flags, s);
}

// The LDS bytes the launches above request, at the seams of their tables: the
// figures of the hand-written sums these launchers held before the layouts
// were shared with the kernels (tests/test_lsap_lds_layout_cpu.py).
static_assert(lsap_i64_lds(1, 1, 1, 10) == 256 && lsap_i64_lds(1, 1, 4, 10) == 256);
static_assert(lsap_i64_lds(64, 64, 1, 10) == 1088 && lsap_i64_lds(64, 64, 4, 10) == 1088);
static_assert(lsap_i64_lds(65, 65, 1, 10) == 1152 && lsap_i64_lds(65, 65, 4, 10) == 1152);
static_assert(lsap_i64_lds(256, 256, 1, 10) == 3776 && lsap_i64_lds(256, 256, 4, 10) == 3776);
static_assert(lsap_i64_lds(257, 257, 1, 10) == 3840 && lsap_i64_lds(257, 257, 4, 10) == 3840);
static_assert(lsap_i64_lds(512, 512, 1, 10) == 7360 && lsap_i64_lds(512, 512, 4, 10) == 7360);
static_assert(lsap_i64_lds(513, 513, 1, 10) == 7424 && lsap_i64_lds(513, 513, 4, 10) == 7424);
static_assert(lsap_i64_lds(1024, 1024, 1, 10) == 14528 && lsap_i64_lds(1024, 1024, 4, 10) == 14528);
static_assert(lsap_i64_lds(1, 1024, 4, 10) == 4320);
static_assert(lsap_i64_lds(1025, 1025, 8, 12) == 14720);
static_assert(lsap_i64_lds(2048, 2048, 8, 12) == 28992);
static_assert(lsap_i64_lds(2049, 2049, 16, 12) == 29376);
static_assert(lsap_i64_lds(3072, 3072, 16, 12) == 43648);
static_assert(lsap_i64_lds(3073, 3073, 16, 12) == 43712);
static_assert(lsap_i64_lds(4096, 4096, 16, 12) == 57984);
static_assert(lsap_i64_lds(1, 4096, 16, 12) == 17056);
static_assert(lsap_f64_lds(1) == 32 && lsap_f64_mw_lds(1, 1, 4, 10) == 160);
static_assert(lsap_f64_lds(64) == 640 && lsap_f64_mw_lds(64, 64, 4, 10) == 992);
static_assert(lsap_f64_lds(65) == 672 && lsap_f64_mw_lds(65, 65, 4, 10) == 1056);
static_assert(lsap_f64_lds(256) == 2560 && lsap_f64_mw_lds(256, 256, 4, 10) == 3680);
static_assert(lsap_f64_lds(257) == 2592 && lsap_f64_mw_lds(257, 257, 4, 10) == 3744);
static_assert(lsap_f64_lds(512) == 5120 && lsap_f64_mw_lds(512, 512, 4, 10) == 7264);
static_assert(lsap_f64_lds(513) == 5152 && lsap_f64_mw_lds(513, 513, 4, 10) == 7328);
static_assert(lsap_f64_lds(1024) == 10240 && lsap_f64_mw_lds(1024, 1024, 4, 10) == 14432);
static_assert(lsap_f64_lds(1) == 32 && lsap_f64_mw_lds(1, 1024, 4, 10) == 4224);
static_assert(lsap_f64_mw_lds(1025, 1025, 8, 12) == 14656);
static_assert(lsap_f64_mw_lds(2048, 2048, 8, 12) == 28928);
static_assert(lsap_f64_mw_lds(2049, 2049, 8, 12) == 28992);
static_assert(lsap_f64_mw_lds(3072, 3072, 8, 12) == 43264);
static_assert(lsap_f64_mw_lds(3073, 3073, 8, 12) == 43328);
static_assert(lsap_f64_mw_lds(4096, 4096, 8, 12) == 57600);
static_assert(lsap_f64_mw_lds(1, 4096, 8, 12) == 16672);

// The lsap_warm_ entries: warm_prep_kernel over the batch, then (unless
// SH_FLAG_BUILD_ONLY) the continuation.  One launch table by the column count
// alone -- the result does not depend on the configuration -- with the cold
// tables' (NW, K, FB) at each size: one wave up to 64 columns, four waves up to
// SH_MAX_N, with_large_cfg / with_large_f64_cfg beyond.  SH_FLAG_F64_MW / _SW
// have nothing to choose between here and are ignored.  The LDS is the cold
// kernels' (the same lists); warm_prep_kernel's stays below LDS_NO_ATTR.
static_assert(warm_prep_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE) == 57344 && warm_prep_lds(1, SH_MAX_N_LARGE) == 32784);
static_assert(warm_prep_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE) <= LDS_NO_ATTR);

template <typename S, typename T>
int launch_warm(const S *C, int nr, int n, int B, const int32_t *shape, int32_t *col, T *cost, T *du, T *dv,
                int32_t *kept, unsigned flags, hipStream_t s) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, SH_MAX_N_LARGE));
  if (!C && B > 0) return fail(SH_ERR_ARGS, "null C");
  if ((!du || !dv) && B > 0) return fail(SH_ERR_ARGS, "null u or v");
  if (B == 0) return SH_OK;
  hipLaunchKernelGGL((warm_prep_kernel<S, T>), dim3(B), dim3(PREP_WG), warm_prep_lds(nr, n), s, C, nr, n, shape, col,
                     du, dv, kept);
  HIP_TRY(hipGetLastError());
  if (flags & SH_FLAG_BUILD_ONLY) return SH_OK;
  auto mw = [&](auto cfg) {
    using C_ = decltype(cfg);
    if constexpr (std::is_same<T, int64_t>::value)
      hipLaunchKernelGGL((warm_i64_kernel<C_::NW, C_::K, S, C_::FB>), dim3(B), dim3(C_::NW * WAVE),
                         lsap_i64_lds(nr, n, C_::NW, C_::FB), s, C, nr, n, shape, col, cost, du, dv, flags);
    else
      hipLaunchKernelGGL((warm_f64_mw_kernel<C_::NW, C_::K, S, C_::FB>), dim3(B), dim3(C_::NW * WAVE),
                         lsap_f64_mw_lds(nr, n, C_::NW, C_::FB), s, C, nr, n, shape, col, cost, du, dv);
    return SH_OK;
  };
  if (n > SH_MAX_N) {
    if constexpr (std::is_same<T, int64_t>::value) with_large_cfg(n, mw);
    else with_large_f64_cfg(n, mw);
  } else if (n > 512) {
    mw(BigCfg<4, 4, 10>{});
  } else if (n > 256) {
    mw(BigCfg<4, 2, 10>{});
  } else if (n > WAVE) {
    mw(BigCfg<4, 1, 10>{});
  } else if constexpr (std::is_same<T, int64_t>::value) {
    mw(BigCfg<1, 1, 10>{});
  } else {
    hipLaunchKernelGGL((warm_f64_kernel<1, S>), dim3(B), dim3(WAVE), lsap_f64_lds(nr), s, C, nr, n, shape, col, cost,
                       du, dv);
  }
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// The lsap_warm_fr_ entries: launch_warm's checks, its two launches and its
// table, with frow_prep_kernel and the frow_ continuations.  The continuations
// hold the padded problem's n rows: their LDS is the square footprint (plus 12
// static bytes a wave).
static_assert(lsap_i64_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE, 16, 12) + 16 * 12 <= LDS_NO_ATTR);
static_assert(lsap_f64_mw_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE, 8, 12) + 8 * 12 <= LDS_NO_ATTR);

template <typename S, typename T>
int launch_warm_fr(const S *C, int nr, int n, int B, const int32_t *shape, int32_t *col, T *cost, T *du, T *dv,
                   int32_t *kept, T *theta, unsigned flags, hipStream_t s) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, SH_MAX_N_LARGE));
  if (!C && B > 0) return fail(SH_ERR_ARGS, "null C");
  if ((!du || !dv) && B > 0) return fail(SH_ERR_ARGS, "null u or v");
  if (B == 0) return SH_OK;
  hipLaunchKernelGGL((frow_prep_kernel<S, T>), dim3(B), dim3(PREP_WG), warm_prep_lds(nr, n), s, C, nr, n, shape, col,
                     du, dv, kept, theta);
  HIP_TRY(hipGetLastError());
  if (flags & SH_FLAG_BUILD_ONLY) return SH_OK;
  auto mw = [&](auto cfg) {
    using C_ = decltype(cfg);
    if constexpr (std::is_same<T, int64_t>::value)
      hipLaunchKernelGGL((frow_i64_kernel<C_::NW, C_::K, S, C_::FB>), dim3(B), dim3(C_::NW * WAVE),
                         lsap_i64_lds(n, n, C_::NW, C_::FB), s, C, nr, n, shape, col, cost, du, dv, theta, flags);
    else
      hipLaunchKernelGGL((frow_f64_mw_kernel<C_::NW, C_::K, S, C_::FB>), dim3(B), dim3(C_::NW * WAVE),
                         lsap_f64_mw_lds(n, n, C_::NW, C_::FB), s, C, nr, n, shape, col, cost, du, dv, theta);
    return SH_OK;
  };
  if (n > SH_MAX_N) {
    if constexpr (std::is_same<T, int64_t>::value) with_large_cfg(n, mw);
    else with_large_f64_cfg(n, mw);
  } else if (n > 512) {
    mw(BigCfg<4, 4, 10>{});
  } else if (n > 256) {
    mw(BigCfg<4, 2, 10>{});
  } else if (n > WAVE) {
    mw(BigCfg<4, 1, 10>{});
  } else if constexpr (std::is_same<T, int64_t>::value) {
    mw(BigCfg<1, 1, 10>{});
  } else {
    hipLaunchKernelGGL((frow_f64_kernel<1, S>), dim3(B), dim3(WAVE), lsap_f64_lds(n), s, C, nr, n, shape, col, cost,
                       du, dv, theta);
  }
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// The lsap_murty_children_ entries and each expansion of lsap_kbest_: the two
// launches of launch_warm over the B * nr children, murty_prep_kernel and then
// the continuation by launch_warm's float table up to SH_MAX_N columns (the
// same (NW, K, FB) and the same LDS lists; the prep's list has one byte a
// column more).  The caller made the checks.  forb_out: where the pool keeps
// each child's F_t, or null.
static_assert(murty_prep_lds(SH_MAX_N, SH_MAX_N) <= LDS_NO_ATTR);

// fr (the _fr_ entries, DESIGN.md §22): the free-rows kernels, whose
// continuations hold the padded problem's n rows.
template <typename S>
int launch_murty(const S *C, int nr, int n, int B, const int32_t *shape, const int32_t *pcol, const double *pv,
                 const int32_t *pp, const uint64_t *forb, int32_t *col, double *cost, double *du, double *dv,
                 int32_t *kept, uint64_t *forb_out, bool fr, hipStream_t s) {
  const dim3 grid((unsigned)((size_t)B * nr));
  if (fr)
    hipLaunchKernelGGL((frow_mprep_kernel<S>), grid, dim3(PREP_WG), murty_prep_lds(nr, n), s, C, nr, n, shape, pcol,
                       pv, pp, forb, col, du, dv, kept, forb_out);
  else
    hipLaunchKernelGGL((murty_prep_kernel<S>), grid, dim3(PREP_WG), murty_prep_lds(nr, n), s, C, nr, n, shape, pcol,
                       pv, pp, forb, col, du, dv, kept, forb_out);
  auto mw = [&](auto cfg) {
    using C_ = decltype(cfg);
    if (fr)
      hipLaunchKernelGGL((frow_mf64_mw_kernel<C_::NW, C_::K, S, C_::FB>), grid, dim3(C_::NW * WAVE),
                         lsap_f64_mw_lds(n, n, C_::NW, C_::FB), s, C, nr, n, shape, pcol, pp, forb, col, cost, du, dv);
    else
      hipLaunchKernelGGL((murty_f64_mw_kernel<C_::NW, C_::K, S, C_::FB>), grid, dim3(C_::NW * WAVE),
                         lsap_f64_mw_lds(nr, n, C_::NW, C_::FB), s, C, nr, n, shape, pcol, pp, forb, col, cost, du,
                         dv);
  };
  if (n > 512) mw(BigCfg<4, 4, 10>{});
  else if (n > 256) mw(BigCfg<4, 2, 10>{});
  else if (n > WAVE) mw(BigCfg<4, 1, 10>{});
  else if (fr)
    hipLaunchKernelGGL((frow_mf64_kernel<1, S>), grid, dim3(WAVE), lsap_f64_lds(n), s, C, nr, n, shape, pcol, pp, forb,
                       col, cost, du, dv);
  else
    hipLaunchKernelGGL((murty_f64_kernel<1, S>), grid, dim3(WAVE), lsap_f64_lds(nr), s, C, nr, n, shape, pcol, pp,
                       forb, col, cost, du, dv);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

int check_murty_sizes(int nr, int nc, int B) {
  if (nr < 1 || nc > SH_MAX_N) return fail(SH_ERR_ARGS, "sizes must be in [1, 1024]");
  if (nr > nc) return fail(SH_ERR_ARGS, "nr > nc: transpose tall input (as scipy does) and solve that");
  if (B < 0) return fail(SH_ERR_ARGS, "B < 0");
  if ((uint64_t)B * (uint64_t)nr > (uint64_t)INT32_MAX) return fail(SH_ERR_ARGS, "B * nr children exceed 2^31 - 1");
  return SH_OK;
}

template <typename S>
int murty_children(const S *C, int nr, int n, int B, const int32_t *shape, const int32_t *pcol, const double *pv,
                   const int32_t *pp, const uint64_t *forb, int32_t *col, double *cost, double *du, double *dv,
                   int32_t *kept, bool fr, hipStream_t s) {
  HIP_TRY_RC(check_murty_sizes(nr, n, B));
  if (B > 0 && (!C || !pcol || !pv || !pp || !forb)) return fail(SH_ERR_ARGS, "null C, pcol, pv, p or forb");
  if (B > 0 && (!col || !cost || !du || !dv)) return fail(SH_ERR_ARGS, "null col, cost, u or v");
  if (B == 0) return SH_OK;
  return launch_murty(C, nr, n, B, shape, pcol, pv, pp, forb, col, cost, du, dv, kept, (uint64_t *)nullptr, fr, s);
}

// The pool of lsap_kbest_ (KbestPool) inside d_work: the 8-byte arrays, then
// the int32 ones.  Returns the bytes, or 0 where they do not fit a size_t.
size_t kbest_carve(unsigned char *base, int nr, int nc, int B, int k, KbestPool *P) {
  const size_t W = (size_t)murty_words(nc), b = (size_t)B, r = (size_t)nr, c = (size_t)nc;
  size_t rounds_nodes;  // (k - 1) * B * nr
  if ((uint64_t)k * (uint64_t)nr > (uint64_t)INT32_MAX) return 0;  // (the pop counts slots in an int)
  if (__builtin_mul_overflow((size_t)(k - 1), b * r, &rounds_nodes)) return 0;
  const size_t per_node = 8 * (1 + c + W) + 4 * r;  // cost, v, F; col
  size_t pool;
  if (__builtin_mul_overflow(rounds_nodes, per_node, &pool)) return 0;
  const size_t fixed = 8 * (b + b * c + b * r * r + b * c + b * W) + 4 * (b * r + b * r + b);
  size_t total;
  if (__builtin_add_overflow(pool, fixed, &total)) return 0;
  if (P) {
    size_t off = 0;
    auto take = [&](auto *&ptr, size_t count) {
      ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + off);
      off += count * sizeof(*ptr);
    };
    take(P->root_cost, b);
    take(P->root_v, b * c);
    take(P->u, b * r * r);
    take(P->cost, rounds_nodes);
    take(P->v, rounds_nodes * c);
    take(P->stage_v, b * c);
    take(P->forb, rounds_nodes * W);
    take(P->stage_forb, b * W);
    take(P->root_col, b * r);
    take(P->col, rounds_nodes * r);
    take(P->stage_col, b * r);
    take(P->stage_p, b);
  }
  return (total + 7) & ~(size_t)7;
}

// lsap_kbest_: the cold solve with duals into the root's slot, then for each
// rank the pop and (but for the last) the expansion of what it popped into
// round r's block: 1 + k + 2 (k - 1) launches, whatever the data.
template <typename S>
int kbest(const S *C, int nr, int n, int B, const int32_t *shape, int k, int32_t *cols, double *costs,
          int32_t *count, void *work, size_t work_bytes, unsigned flags, bool fr, hipStream_t s) {
  HIP_TRY_RC(check_murty_sizes(nr, n, B));
  if (k < 1) return fail(SH_ERR_ARGS, "k < 1");
  if ((uint64_t)k * (uint64_t)nr > (uint64_t)INT32_MAX) return fail(SH_ERR_ARGS, "k * nr exceeds 2^31 - 1");
  if (B > 0 && (!C || !cols || !costs || !count || !work)) return fail(SH_ERR_ARGS, "null C, cols, costs, count or work");
  const size_t need = B > 0 ? kbest_carve(nullptr, nr, n, B, k, nullptr) : 0;
  if (B > 0 && (need == 0 || work_bytes < need)) return fail(SH_ERR_ARGS, "work_bytes < lsap_kbest_work_bytes");
  if ((uintptr_t)work % 8 != 0) return fail(SH_ERR_ARGS, "d_work must be 8-byte aligned");
  HIP_TRY_RC(check_f64_flags(flags, n));
  if (B == 0) return SH_OK;
  KbestPool P;
  kbest_carve((unsigned char *)work, nr, n, B, k, &P);
  HIP_TRY_RC(solve_f64(C, nr, n, B, shape, P.root_col, P.root_cost, P.u, P.root_v, flags, s));
  const size_t bn = (size_t)B * nr, W = (size_t)murty_words(n);
  for (int r = 0; r < k; ++r) {
    hipLaunchKernelGGL(kbest_pop_kernel, dim3(B), dim3(KBEST_POP_WG), 0, s, P, nr, n, B, r, k, cols, costs, count);
    if (r == k - 1) break;
    HIP_TRY_RC(launch_murty(C, nr, n, B, shape, P.stage_col, P.stage_v, P.stage_p, P.stage_forb,
                            P.col + r * bn * nr, P.cost + r * bn, P.u, P.v + r * bn * n, (int32_t *)nullptr,
                            P.forb + r * bn * W, fr, s));
  }
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// The certificate (lsap_cert_kernel, lsap_slack_kernel, lsap_cert_final_kernel):
// S the stored cost type, T int64_t or double.  The pass over the corners
// reads 16 bytes per load when every row starts 16-byte aligned; a batch too
// small to fill the chip with one workgroup per instance is split by rows.
// cap: the entry's limit, SH_MAX_N or SH_MAX_N_LARGE.  The kernels' column
// capacity NCAP is SH_MAX_N up to that many columns whatever the entry (the
// same kernels, the same bits), SH_MAX_N_LARGE beyond.
template <typename S, typename T>
int launch_lsap_check(const S *C, int nr, int n, int B, int cap, const int32_t *shape, const int32_t *col,
                      const T *u, const T *v, T *slack, int32_t *flg, hipStream_t s) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, cap));
  if (B > 0 && (!C || !u || !v || !slack || !flg)) return fail(SH_ERR_ARGS, "null C, u, v, slack or flags");
  if (B == 0) return SH_OK;
  auto go = [&](auto ncap) {
    constexpr int NCAP = decltype(ncap)::value;
    hipLaunchKernelGGL((lsap_cert_kernel<S, T, NCAP>), dim3(B), dim3(CERT_WG), 0, s, C, nr, n, shape, col, u, v,
                       slack, flg);
    // at least 8 rows per workgroup, about 2048 workgroups when the batch allows
    const int chunks = std::min(std::max(1, 2048 / B), (nr + 7) / 8);
    const int rows_per = (nr + chunks - 1) / chunks;
    const dim3 grid(B, (nr + rows_per - 1) / rows_per);
    constexpr int VEC = 16 / (int)sizeof(S);
    if ((uintptr_t)C % 16 == 0 && n % VEC == 0)
      hipLaunchKernelGGL((lsap_slack_kernel<S, T, VEC, NCAP>), grid, dim3(CERT_WG), 0, s, C, nr, n, shape, u, v,
                         slack, flg, rows_per);
    else
      hipLaunchKernelGGL((lsap_slack_kernel<S, T, 1, NCAP>), grid, dim3(CERT_WG), 0, s, C, nr, n, shape, u, v,
                         slack, flg, rows_per);
  };
  if (n <= SH_MAX_N) go(int_c<SH_MAX_N>{});
  else go(int_c<SH_MAX_N_LARGE>{});
  hipLaunchKernelGGL((lsap_cert_final_kernel<T>), dim3((B + CERT_WG - 1) / CERT_WG), dim3(CERT_WG), 0, s,
                     B, slack, flg);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// ---------------------------------------------------------------------------
// The lsap_solve_csr_ entries: the float solvers on CSR costs (CsrLoader).
// d_work holds what lsap_csr_prep_kernel writes for the B * nr rows: the
// 64-bit masks of their ceil(nc / 64) words, then the words' 16-bit prefixes.
// ---------------------------------------------------------------------------
size_t csr_words(int nr, int nc, int B) { return (size_t)B * (size_t)nr * (size_t)((nc + 63) / 64); }

// Two launches on the stream: the prep, then launch_f64's table with the CSR
// kernels.  Every check, launch_f64's among them, precedes the first launch.
template <typename S>
int launch_lsap_csr(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                    const int32_t *shape, int32_t *col, double *cost, double *du, double *dv, void *work,
                    size_t work_bytes, unsigned flags, hipStream_t s) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, SH_MAX_N_LARGE));
  if (!indptr && B > 0) return fail(SH_ERR_ARGS, "null indptr");
  if ((du == nullptr) != (dv == nullptr)) return fail(SH_ERR_ARGS, "u and v: both or neither");
  HIP_TRY_RC(check_f64_flags(flags, n));
  if (work_bytes < lsap_csr_work_bytes(nr, n, B) || (B > 0 && !work))
    return fail(SH_ERR_ARGS, "work buffer smaller than lsap_csr_work_bytes");
  if ((uintptr_t)work % 8) return fail(SH_ERR_ARGS, "work buffer not 8-byte aligned");
  const int64_t rows = (int64_t)B * nr;
  constexpr int PREP_ROWS = CSR_PREP_WG / WAVE;
  if ((rows + PREP_ROWS - 1) / PREP_ROWS > INT32_MAX) return fail(SH_ERR_ARGS, "B * nr too large");
  if (B == 0) return SH_OK;
  uint64_t *mask = (uint64_t *)work;
  uint16_t *pre = (uint16_t *)(mask + csr_words(nr, n, B));
  hipLaunchKernelGGL(lsap_csr_prep_kernel, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(CSR_PREP_WG),
                     0, s, indptr, indices, nr, n, rows, shape, mask, pre);
  if (flags & SH_FLAG_BUILD_ONLY) {  // (phase timing: the prep alone)
    HIP_TRY(hipGetLastError());
    return SH_OK;
  }
  return launch_f64(CsrF64<S>{indptr, data, mask, pre}, nr, n, B, shape, col, cost, du, dv, flags, s);
}

// The lsap_warm_csr_ entries (DESIGN.md §19): three launches on the stream,
// the prep above, warm_csr_prep_kernel and (unless SH_FLAG_BUILD_ONLY, which
// here has launch_warm's meaning: the start state) the continuation by
// launch_warm's float table, which goes by the column count alone.
// SH_FLAG_F64_MW / _SW are ignored.  Every check precedes the first launch.
template <typename S>
int launch_warm_csr(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                    const int32_t *shape, int32_t *col, double *cost, double *du, double *dv, int32_t *kept,
                    void *work, size_t work_bytes, unsigned flags, hipStream_t s) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, SH_MAX_N_LARGE));
  if (!indptr && B > 0) return fail(SH_ERR_ARGS, "null indptr");
  if ((!du || !dv) && B > 0) return fail(SH_ERR_ARGS, "null u or v");
  if (work_bytes < lsap_csr_work_bytes(nr, n, B) || (B > 0 && !work))
    return fail(SH_ERR_ARGS, "work buffer smaller than lsap_csr_work_bytes");
  if ((uintptr_t)work % 8) return fail(SH_ERR_ARGS, "work buffer not 8-byte aligned");
  const int64_t rows = (int64_t)B * nr;
  constexpr int PREP_ROWS = CSR_PREP_WG / WAVE;
  if ((rows + PREP_ROWS - 1) / PREP_ROWS > INT32_MAX) return fail(SH_ERR_ARGS, "B * nr too large");
  if (B == 0) return SH_OK;
  uint64_t *mask = (uint64_t *)work;
  uint16_t *pre = (uint16_t *)(mask + csr_words(nr, n, B));
  hipLaunchKernelGGL(lsap_csr_prep_kernel, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(CSR_PREP_WG),
                     0, s, indptr, indices, nr, n, rows, shape, mask, pre);
  hipLaunchKernelGGL((warm_csr_prep_kernel<S>), dim3(B), dim3(PREP_WG), warm_prep_lds(nr, n), s, indptr, data, mask,
                     pre, nr, n, shape, col, du, dv, kept);
  HIP_TRY(hipGetLastError());
  if (flags & SH_FLAG_BUILD_ONLY) return SH_OK;
  auto mw = [&](auto cfg) {
    using C_ = decltype(cfg);
    hipLaunchKernelGGL((warm_csr_mw_kernel<C_::NW, C_::K, S, C_::FB>), dim3(B), dim3(C_::NW * WAVE),
                       lsap_f64_mw_lds(nr, n, C_::NW, C_::FB), s, indptr, data, mask, pre, nr, n, shape, col, cost, du,
                       dv);
    return SH_OK;
  };
  if (n > SH_MAX_N) with_large_f64_cfg(n, mw);
  else if (n > 512) mw(BigCfg<4, 4, 10>{});
  else if (n > 256) mw(BigCfg<4, 2, 10>{});
  else if (n > WAVE) mw(BigCfg<4, 1, 10>{});
  else
    hipLaunchKernelGGL((warm_csr_kernel<1, S>), dim3(B), dim3(WAVE), lsap_f64_lds(nr), s, indptr, data, mask, pre, nr,
                       n, shape, col, cost, du, dv);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// The lsap_warm_fr_csr_ entries (DESIGN.md §23): launch_warm_csr's checks, its
// three launches and its table, with fcsr_prep_kernel and the fcsr_
// continuations.  The continuations hold the padded problem's n rows: their LDS
// is the square footprint (plus frow_virtual_rows' 12 static bytes a wave).
static_assert(lsap_f64_mw_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE, 8, 12) + 8 * 12 <= LDS_NO_ATTR);
static_assert(lsap_f64_lds(WAVE) <= LDS_NO_ATTR);

template <typename S>
int launch_warm_fr_csr(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                       const int32_t *shape, int32_t *col, double *cost, double *du, double *dv, int32_t *kept,
                       double *theta, void *work, size_t work_bytes, unsigned flags, hipStream_t s) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, SH_MAX_N_LARGE));
  if (!indptr && B > 0) return fail(SH_ERR_ARGS, "null indptr");
  if ((!du || !dv) && B > 0) return fail(SH_ERR_ARGS, "null u or v");
  if (work_bytes < lsap_csr_work_bytes(nr, n, B) || (B > 0 && !work))
    return fail(SH_ERR_ARGS, "work buffer smaller than lsap_csr_work_bytes");
  if ((uintptr_t)work % 8) return fail(SH_ERR_ARGS, "work buffer not 8-byte aligned");
  const int64_t rows = (int64_t)B * nr;
  constexpr int PREP_ROWS = CSR_PREP_WG / WAVE;
  if ((rows + PREP_ROWS - 1) / PREP_ROWS > INT32_MAX) return fail(SH_ERR_ARGS, "B * nr too large");
  if (B == 0) return SH_OK;
  uint64_t *mask = (uint64_t *)work;
  uint16_t *pre = (uint16_t *)(mask + csr_words(nr, n, B));
  hipLaunchKernelGGL(lsap_csr_prep_kernel, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(CSR_PREP_WG),
                     0, s, indptr, indices, nr, n, rows, shape, mask, pre);
  hipLaunchKernelGGL((fcsr_prep_kernel<S>), dim3(B), dim3(PREP_WG), warm_prep_lds(nr, n), s, indptr, data, mask, pre,
                     nr, n, shape, col, du, dv, kept, theta);
  HIP_TRY(hipGetLastError());
  if (flags & SH_FLAG_BUILD_ONLY) return SH_OK;
  auto mw = [&](auto cfg) {
    using C_ = decltype(cfg);
    hipLaunchKernelGGL((fcsr_mw_kernel<C_::NW, C_::K, S, C_::FB>), dim3(B), dim3(C_::NW * WAVE),
                       lsap_f64_mw_lds(n, n, C_::NW, C_::FB), s, indptr, data, mask, pre, nr, n, shape, col, cost, du,
                       dv, theta);
    return SH_OK;
  };
  if (n > SH_MAX_N) with_large_f64_cfg(n, mw);
  else if (n > 512) mw(BigCfg<4, 4, 10>{});
  else if (n > 256) mw(BigCfg<4, 2, 10>{});
  else if (n > WAVE) mw(BigCfg<4, 1, 10>{});
  else
    hipLaunchKernelGGL((fcsr_kernel<1, S>), dim3(B), dim3(WAVE), lsap_f64_lds(n), s, indptr, data, mask, pre, nr, n,
                       shape, col, cost, du, dv, theta);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// ---------------------------------------------------------------------------
// k-best on the CSR (DESIGN.md §21): the lsap_murty_children_csr_ and
// lsap_kbest_csr_ entries.  launch_mcsr is launch_murty behind the masking CSR
// loader, after lsap_csr_prep_kernel: mcsr_prep_kernel and then the
// continuation by the same table on the column count alone.  The caller made
// the checks and ran the prep.
// ---------------------------------------------------------------------------
static_assert(mcsr_prep_lds(SH_MAX_N, SH_MAX_N) <= LDS_NO_ATTR);

// fr (the _fr_csr_ entries, DESIGN.md §23): the free-rows kernels, whose
// continuations hold the padded problem's n rows.
template <typename S>
int launch_mcsr(const int64_t *indptr, const S *data, const uint64_t *mask, const uint16_t *pre, int nr, int n, int B,
                const int32_t *shape, const int32_t *pcol, const double *pv, const int32_t *pp, const uint64_t *forb,
                int32_t *col, double *cost, double *du, double *dv, int32_t *kept, uint64_t *forb_out, bool fr,
                hipStream_t s) {
  const dim3 grid((unsigned)((size_t)B * nr));
  if (fr)
    hipLaunchKernelGGL((fcsr_mprep_kernel<S>), grid, dim3(PREP_WG), mcsr_prep_lds(nr, n), s, indptr, data, mask, pre,
                       nr, n, shape, pcol, pv, pp, forb, col, du, dv, kept, forb_out);
  else
    hipLaunchKernelGGL((mcsr_prep_kernel<S>), grid, dim3(PREP_WG), mcsr_prep_lds(nr, n), s, indptr, data, mask, pre,
                       nr, n, shape, pcol, pv, pp, forb, col, du, dv, kept, forb_out);
  auto mw = [&](auto cfg) {
    using C_ = decltype(cfg);
    if (fr)
      hipLaunchKernelGGL((fcsr_mf64_mw_kernel<C_::NW, C_::K, S, C_::FB>), grid, dim3(C_::NW * WAVE),
                         lsap_f64_mw_lds(n, n, C_::NW, C_::FB), s, indptr, data, mask, pre, nr, n, shape, pcol, pp,
                         forb, col, cost, du, dv);
    else
      hipLaunchKernelGGL((mcsr_f64_mw_kernel<C_::NW, C_::K, S, C_::FB>), grid, dim3(C_::NW * WAVE),
                         lsap_f64_mw_lds(nr, n, C_::NW, C_::FB), s, indptr, data, mask, pre, nr, n, shape, pcol, pp,
                         forb, col, cost, du, dv);
  };
  if (n > 512) mw(BigCfg<4, 4, 10>{});
  else if (n > 256) mw(BigCfg<4, 2, 10>{});
  else if (n > WAVE) mw(BigCfg<4, 1, 10>{});
  else if (fr)
    hipLaunchKernelGGL((fcsr_mf64_kernel<1, S>), grid, dim3(WAVE), lsap_f64_lds(n), s, indptr, data, mask, pre, nr, n,
                       shape, pcol, pp, forb, col, cost, du, dv);
  else
    hipLaunchKernelGGL((mcsr_f64_kernel<1, S>), grid, dim3(WAVE), lsap_f64_lds(nr), s, indptr, data, mask, pre, nr, n,
                       shape, pcol, pp, forb, col, cost, du, dv);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// The bitmap pass of a batch whose sizes check_murty_sizes accepted (B * nr
// rows fit an int, so the grid does).
void launch_csr_prep(const int64_t *indptr, const int32_t *indices, int nr, int n, int B, const int32_t *shape,
                     uint64_t *mask, uint16_t *pre, hipStream_t s) {
  const int64_t rows = (int64_t)B * nr;
  constexpr int PREP_ROWS = CSR_PREP_WG / WAVE;
  hipLaunchKernelGGL(lsap_csr_prep_kernel, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(CSR_PREP_WG),
                     0, s, indptr, indices, nr, n, rows, shape, mask, pre);
}

template <typename S>
int murty_children_csr(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                       const int32_t *shape, const int32_t *pcol, const double *pv, const int32_t *pp,
                       const uint64_t *forb, int32_t *col, double *cost, double *du, double *dv, int32_t *kept,
                       void *work, size_t work_bytes, bool fr, hipStream_t s) {
  HIP_TRY_RC(check_murty_sizes(nr, n, B));
  if (B > 0 && (!indptr || !pcol || !pv || !pp || !forb)) return fail(SH_ERR_ARGS, "null indptr, pcol, pv, p or forb");
  if (B > 0 && (!col || !cost || !du || !dv)) return fail(SH_ERR_ARGS, "null col, cost, u or v");
  if (B > 0 && (!work || work_bytes < lsap_csr_work_bytes(nr, n, B)))
    return fail(SH_ERR_ARGS, "work buffer smaller than lsap_csr_work_bytes");
  if ((uintptr_t)work % 8) return fail(SH_ERR_ARGS, "work buffer not 8-byte aligned");
  if (B == 0) return SH_OK;
  uint64_t *mask = (uint64_t *)work;
  uint16_t *pre = (uint16_t *)(mask + csr_words(nr, n, B));
  launch_csr_prep(indptr, indices, nr, n, B, shape, mask, pre, s);
  return launch_mcsr(indptr, data, mask, pre, nr, n, B, shape, pcol, pv, pp, forb, col, cost, du, dv, kept,
                     (uint64_t *)nullptr, fr, s);
}

// d_work of lsap_kbest_csr_: the dense pool (kbest_carve), then the words of
// lsap_csr_prep_kernel.  Returns 0 where the pool does not fit a size_t.
size_t kbest_csr_bytes(int nr, int nc, int B, int k, size_t *pool_bytes) {
  const size_t pool = kbest_carve(nullptr, nr, nc, B, k, nullptr);  // (a multiple of 8)
  size_t total;
  if (B < 1 || pool == 0 || __builtin_add_overflow(pool, lsap_csr_work_bytes(nr, nc, B), &total)) return 0;
  if (pool_bytes) *pool_bytes = pool;
  return (total + 7) & ~(size_t)7;
}

// lsap_kbest_csr_: the bitmap pass and the cold CSR solve with duals into the
// root's slot (launch_lsap_csr), then kbest's loop with launch_mcsr on the same
// words: 2 + k + 2 (k - 1) = 3 k launches, whatever the data.
template <typename S>
int kbest_csr(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
              const int32_t *shape, int k, int32_t *cols, double *costs, int32_t *count, void *work,
              size_t work_bytes, unsigned flags, bool fr, hipStream_t s) {
  HIP_TRY_RC(check_murty_sizes(nr, n, B));
  if (k < 1) return fail(SH_ERR_ARGS, "k < 1");
  if ((uint64_t)k * (uint64_t)nr > (uint64_t)INT32_MAX) return fail(SH_ERR_ARGS, "k * nr exceeds 2^31 - 1");
  if (B > 0 && (!indptr || !cols || !costs || !count || !work))
    return fail(SH_ERR_ARGS, "null indptr, cols, costs, count or work");
  size_t pool = 0;
  const size_t need = B > 0 ? kbest_csr_bytes(nr, n, B, k, &pool) : 0;
  if (B > 0 && (need == 0 || work_bytes < need)) return fail(SH_ERR_ARGS, "work_bytes < lsap_kbest_csr_work_bytes");
  if ((uintptr_t)work % 8 != 0) return fail(SH_ERR_ARGS, "d_work must be 8-byte aligned");
  HIP_TRY_RC(check_f64_flags(flags, n));
  if (B == 0) return SH_OK;
  KbestPool P;
  kbest_carve((unsigned char *)work, nr, n, B, k, &P);
  uint64_t *mask = (uint64_t *)((unsigned char *)work + pool);
  uint16_t *pre = (uint16_t *)(mask + csr_words(nr, n, B));
  HIP_TRY_RC(launch_lsap_csr(indptr, indices, data, nr, n, B, shape, P.root_col, P.root_cost, P.u, P.root_v, mask,
                             need - pool, flags & (SH_FLAG_F64_MW | SH_FLAG_F64_SW), s));
  const size_t bn = (size_t)B * nr, W = (size_t)murty_words(n);
  for (int r = 0; r < k; ++r) {
    hipLaunchKernelGGL(kbest_pop_kernel, dim3(B), dim3(KBEST_POP_WG), 0, s, P, nr, n, B, r, k, cols, costs, count);
    if (r == k - 1) break;
    HIP_TRY_RC(launch_mcsr(indptr, data, mask, pre, nr, n, B, shape, P.stage_col, P.stage_v, P.stage_p, P.stage_forb,
                           P.col + r * bn * nr, P.cost + r * bn, P.u, P.v + r * bn * n, (int32_t *)nullptr,
                           P.forb + r * bn * W, fr, s));
  }
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// ---------------------------------------------------------------------------
// The certificates on the CSR (DESIGN.md §18): lsap_check_duals_csr_
// (csr_cert_kernel, csr_slack_kernel, lsap_cert_final_kernel), lsap_match_csr_
// (csr_edges_kernel into d_work, then csr_match_kernel) and
// lsap_check_hall_csr_ (csr_hall_check_kernel).
// The sizes and indptr are checked as on lsap_solve_csr_; `out` is the entry's
// first required array (check_lsap_args names it col).
// ---------------------------------------------------------------------------
int check_csr_args(const int64_t *indptr, int nr, int n, int B, const void *out) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, (const int32_t *)out, SH_MAX_N_LARGE));
  if (!indptr && B > 0) return fail(SH_ERR_ARGS, "null indptr");
  return SH_OK;
}

template <typename S>
int launch_csr_cert(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                    const int32_t *shape, const int32_t *col, const double *u, const double *v, double *slack,
                    int32_t *flg, hipStream_t s) {
  HIP_TRY_RC(check_csr_args(indptr, nr, n, B, col));
  if (B > 0 && (!u || !v || !slack || !flg)) return fail(SH_ERR_ARGS, "null u, v, slack or flags");
  if (B == 0) return SH_OK;
  static_assert(csr_cert_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE) + 512 <= 65536, "csr_cert_kernel's LDS");
  hipLaunchKernelGGL((csr_cert_kernel<S>), dim3(B), dim3(CSR_CERT_WG), csr_cert_lds(nr, n), s, indptr, indices, data,
                     nr, n, shape, col, u, v, slack, flg);
  // launch_lsap_check's split: about 2048 workgroups when the batch allows, CSR_SLACK_ROWS rows each at least
  const int chunks = std::min(std::max(1, 2048 / B), (nr + CSR_SLACK_ROWS - 1) / CSR_SLACK_ROWS);
  const int rows_per = (nr + chunks - 1) / chunks;
  hipLaunchKernelGGL((csr_slack_kernel<S>), dim3(B, (nr + rows_per - 1) / rows_per), dim3(CERT_WG), (size_t)n * 8, s,
                     indptr, indices, data, nr, n, shape, u, v, slack, flg, rows_per);
  hipLaunchKernelGGL((lsap_cert_final_kernel<double>), dim3((B + CERT_WG - 1) / CERT_WG), dim3(CERT_WG), 0, s, B,
                     slack, flg);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

template <typename S>
int launch_csr_match(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                     const int32_t *shape, int32_t *match, int32_t *card, uint8_t *wit, void *work,
                     size_t work_bytes, hipStream_t s) {
  HIP_TRY_RC(check_csr_args(indptr, nr, n, B, match));
  if (B > 0 && (!card || !wit)) return fail(SH_ERR_ARGS, "null card or wit");
  if (work_bytes < lsap_csr_work_bytes(nr, n, B) || (B > 0 && !work))
    return fail(SH_ERR_ARGS, "work buffer smaller than lsap_csr_work_bytes");
  if ((uintptr_t)work % 8) return fail(SH_ERR_ARGS, "work buffer not 8-byte aligned");
  const int64_t rows = (int64_t)B * nr;
  constexpr int PREP_ROWS = CSR_PREP_WG / WAVE;
  if ((rows + PREP_ROWS - 1) / PREP_ROWS > INT32_MAX) return fail(SH_ERR_ARGS, "B * nr too large");
  if (B == 0) return SH_OK;
  static_assert(csr_match_lds(SH_MAX_N_LARGE, SH_MAX_N_LARGE) <= 65536, "csr_match_kernel's LDS");
  uint64_t *mask = (uint64_t *)work;  // (the first 8 of lsap_csr_work_bytes' 10 bytes a word)
  hipLaunchKernelGGL((csr_edges_kernel<S>), dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(CSR_PREP_WG),
                     0, s, indptr, indices, data, nr, n, rows, shape, mask);
  hipLaunchKernelGGL(csr_match_kernel, dim3(B), dim3(WAVE), csr_match_lds(nr, n), s, mask, nr, n, shape, match, card,
                     wit);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

template <typename S>
int launch_csr_hall_check(const int64_t *indptr, const int32_t *indices, const S *data, int nr, int n, int B,
                          const int32_t *shape, const int32_t *match, const uint8_t *wit, int32_t *counts,
                          int32_t *flg, hipStream_t s) {
  HIP_TRY_RC(check_csr_args(indptr, nr, n, B, match));
  if (B > 0 && (!wit || !counts || !flg)) return fail(SH_ERR_ARGS, "null wit, counts or flags");
  if (B == 0) return SH_OK;
  hipLaunchKernelGGL((csr_hall_check_kernel<S>), dim3(B), dim3(CERT_WG), 0, s, indptr, indices, data, nr, n, shape,
                     match, wit, counts, flg);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}

// ---------------------------------------------------------------------------
// The lbap_solve_ entries (bottleneck assignment, lbap_kernel).
// ---------------------------------------------------------------------------
// Whether a batch of B instances with nc columns runs the multi-wave design by
// default (measured: DESIGN §15, profiles/lbap.jsonl; four dtypes, 16 / 256 /
// 4096 instances, the multi-wave time over the one-wave time or back).  Up to
// 256 columns one wave won or tied everywhere (128 columns: 25-55 % up to 256
// instances, 2.4-2.6x at 4096; 256 columns: 0-17 %, 1.6-1.9x at 4096).  At
// 1024 columns four waves won everywhere (42-87 % up to 256 instances, 4-13 %
// at 4096).  At 512 columns four waves won up to 1024 instances (5-42 %) and
// one wave from 2048 (4-17 %; 27-54 % at 4096).
bool lbap_mw_default(int nc, int B) { return nc > 512 || (nc > 256 && B <= 1024); }

// The one launch table of lbap_kernel, for the six dtypes DT (LBAP_*); every
// check precedes the launch.  One wave with pick_k's columns a lane up to
// SH_MAX_N columns, or four waves with 1 / 2 / 4 columns a thread (the float
// LSAP table's), eight and sixteen waves with four beyond SH_MAX_N.
int check_lbap_args(const void *C, int nr, int n, int B, const int32_t *col, unsigned flags) {
  HIP_TRY_RC(check_lsap_args(nr, n, B, col, SH_MAX_N_LARGE));
  if (!C && B > 0) return fail(SH_ERR_ARGS, "null C");
  if ((flags & SH_FLAG_LBAP_MW) && (flags & SH_FLAG_LBAP_SW))
    return fail(SH_ERR_ARGS, "SH_FLAG_LBAP_MW and SH_FLAG_LBAP_SW exclude each other");
  if ((flags & SH_FLAG_LBAP_SW) && n > SH_MAX_N)
    return fail(SH_ERR_ARGS, "SH_FLAG_LBAP_SW: no one-wave kernel above 1024 columns");
  return SH_OK;
}

// WIT: the lbap_solve_wit_ entries, bneck_wit_kernel through the same table
// and switch, with `wit` and its own LDS list.
template <int DT, bool WIT = false>
int launch_lbap(const void *C, int nr, int n, int B, const int32_t *shape, int32_t *col, void *value,
                unsigned flags, hipStream_t s, uint8_t *wit = nullptr) {
  HIP_TRY_RC(check_lbap_args(C, nr, n, B, col, flags));
  if (WIT && !wit && B > 0) return fail(SH_ERR_ARGS, "null wit");
  if (B == 0) return SH_OK;
  auto go = [&](auto cfg) {
    using C_ = decltype(cfg);
    if constexpr (WIT)
      hipLaunchKernelGGL((bneck_wit_kernel<C_::NW, C_::K, DT>), dim3(B), dim3(C_::NW * WAVE),
                         lbap_wit_lds(nr, n, C_::NW), s, C, nr, n, shape, col, value, wit, flags);
    else
      hipLaunchKernelGGL((lbap_kernel<C_::NW, C_::K, DT>), dim3(B), dim3(C_::NW * WAVE), lbap_lds(nr, n, C_::NW), s,
                         C, nr, n, shape, col, value, flags);
    HIP_TRY(hipGetLastError());
    return SH_OK;
  };
  const bool mw = n > SH_MAX_N || (!(flags & SH_FLAG_LBAP_SW) && ((flags & SH_FLAG_LBAP_MW) || lbap_mw_default(n, B)));
  if (!mw) {
    switch (pick_k(n)) {
      case 1: return go(BigCfg<1, 1, 0>{});
      case 2: return go(BigCfg<1, 2, 0>{});
      case 4: return go(BigCfg<1, 4, 0>{});
      case 8: return go(BigCfg<1, 8, 0>{});
      default: return go(BigCfg<1, 16, 0>{});
    }
  }
  if (n <= 256) return go(BigCfg<4, 1, 0>{});
  if (n <= 512) return go(BigCfg<4, 2, 0>{});
  if (n <= 1024) return go(BigCfg<4, 4, 0>{});
  if (n <= 2048) return go(BigCfg<8, 4, 0>{});
  return go(BigCfg<16, 4, 0>{});
}

// lbap_lds at the seams of the table above, each region rounded up to 16
// bytes: 16 NW and 8 NW of step slots, 2 nr of col4row, 2 n each of row4col
// and path.
static_assert(lbap_lds(1, 1, 1) == 80 && lbap_lds(64, 64, 1) == 416 && lbap_lds(65, 65, 1) == 464);
static_assert(lbap_lds(128, 128, 1) == 800 && lbap_lds(129, 129, 1) == 848);
static_assert(lbap_lds(256, 256, 1) == 1568 && lbap_lds(257, 257, 1) == 1616);
static_assert(lbap_lds(512, 512, 1) == 3104 && lbap_lds(513, 513, 1) == 3152);
static_assert(lbap_lds(1024, 1024, 1) == 6176);
static_assert(lbap_lds(1, 1, 4) == 144 && lbap_lds(256, 256, 4) == 1632 && lbap_lds(257, 257, 4) == 1680);
static_assert(lbap_lds(512, 512, 4) == 3168 && lbap_lds(513, 513, 4) == 3216);
static_assert(lbap_lds(1024, 1024, 4) == 6240 && lbap_lds(1025, 1025, 8) == 6384);
static_assert(lbap_lds(2048, 2048, 8) == 12480 && lbap_lds(2049, 2049, 16) == 12720);
static_assert(lbap_lds(4096, 4096, 16) == 24960 && lbap_lds(1, 4096, 16) == 16784);
// lbap_wit_lds at the same seams: the list above and 2 nr of stamp.
static_assert(lbap_wit_lds(1, 1, 1) == 96 && lbap_wit_lds(64, 64, 1) == 544 && lbap_wit_lds(65, 65, 1) == 608);
static_assert(lbap_wit_lds(128, 128, 1) == 1056 && lbap_wit_lds(129, 129, 1) == 1120);
static_assert(lbap_wit_lds(256, 256, 1) == 2080 && lbap_wit_lds(257, 257, 1) == 2144);
static_assert(lbap_wit_lds(512, 512, 1) == 4128 && lbap_wit_lds(513, 513, 1) == 4192);
static_assert(lbap_wit_lds(1024, 1024, 1) == 8224);
static_assert(lbap_wit_lds(1, 1, 4) == 160 && lbap_wit_lds(256, 256, 4) == 2144 && lbap_wit_lds(257, 257, 4) == 2208);
static_assert(lbap_wit_lds(512, 512, 4) == 4192 && lbap_wit_lds(513, 513, 4) == 4256);
static_assert(lbap_wit_lds(1024, 1024, 4) == 8288 && lbap_wit_lds(1025, 1025, 8) == 8448);
static_assert(lbap_wit_lds(2048, 2048, 8) == 16576 && lbap_wit_lds(2049, 2049, 16) == 16832);
static_assert(lbap_wit_lds(4096, 4096, 16) == 33152 && lbap_wit_lds(1, 4096, 16) == 16800);

// The lbap_check_ entries (bneck_check_kernel): lbap_solve_'s checks, then one
// launch of one workgroup per instance.
template <int DT>
int launch_lbap_check(const void *C, int nr, int n, int B, const int32_t *shape, const int32_t *col,
                      const void *value, const uint8_t *wit, int32_t *counts, int32_t *flg, unsigned flags,
                      hipStream_t s) {
  HIP_TRY_RC(check_lbap_args(C, nr, n, B, col, flags));
  if (B > 0 && (!value || !wit || !counts || !flg)) return fail(SH_ERR_ARGS, "null value, wit, counts or flags");
  if (B == 0) return SH_OK;
  hipLaunchKernelGGL((bneck_check_kernel<DT>), dim3(B), dim3(CERT_WG), 0, s, C, nr, n, shape, col, value, wit,
                     counts, flg, flags);
  HIP_TRY(hipGetLastError());
  return SH_OK;
}
}  // namespace

extern "C" {

// The five entries of a dense cost type: CT its C-ABI type, KT the kernels'
// element type, T the type of costs and duals, SOLVE solve_i64 or solve_f64.
// nr x nc instances, nr <= nc (the square entries below: nr == nc, no
// shapes).  Every check is on the host and precedes the first device call.
// The _rect_ and _duals_ entries go up to SH_MAX_N columns; the _large_ ones
// up to SH_MAX_N_LARGE, with the same kernels and bits up to SH_MAX_N and the
// FB = 12 instantiations beyond.
#define SH_LSAP_ENTRIES(SUF, CT, KT, T, SOLVE)                                                                  \
  int lsap_solve_batched_rect_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape,               \
                                    int32_t *d_col, T *d_cost, unsigned flags, void *stream) {                  \
    HIP_TRY_RC(check_solve<T>(d_C, nr, nc, B, d_col, false, nullptr, nullptr));                                 \
    return SOLVE((const KT *)d_C, nr, nc, B, d_shape, d_col, d_cost, (T *)nullptr, (T *)nullptr, flags,         \
                 (hipStream_t)stream);                                                                          \
  }                                                                                                             \
  int lsap_solve_batched_duals_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape,              \
                                     int32_t *d_col, T *d_cost, T *d_u, T *d_v, unsigned flags, void *stream) { \
    HIP_TRY_RC(check_solve<T>(d_C, nr, nc, B, d_col, true, d_u, d_v));                                          \
    return SOLVE((const KT *)d_C, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, flags, (hipStream_t)stream);     \
  }                                                                                                             \
  int lsap_solve_large_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape, int32_t *d_col,      \
                             T *d_cost, T *d_u, T *d_v, unsigned flags, void *stream) {                         \
    HIP_TRY_RC(check_large_solve<T>(d_C, nr, nc, B, d_col, d_u, d_v));                                          \
    return SOLVE((const KT *)d_C, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, flags, (hipStream_t)stream);     \
  }                                                                                                             \
  int lsap_check_duals_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape,                      \
                             const int32_t *d_col, const T *d_u, const T *d_v, T *d_slack, int32_t *d_flags,    \
                             void *stream) {                                                                    \
    return launch_lsap_check((const KT *)d_C, nr, nc, B, SH_MAX_N, d_shape, d_col, d_u, d_v, d_slack, d_flags,  \
                             (hipStream_t)stream);                                                              \
  }                                                                                                             \
  int lsap_check_duals_large_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape,                \
                                   const int32_t *d_col, const T *d_u, const T *d_v, T *d_slack,                \
                                   int32_t *d_flags, void *stream) {                                            \
    return launch_lsap_check((const KT *)d_C, nr, nc, B, SH_MAX_N_LARGE, d_shape, d_col, d_u, d_v, d_slack,     \
                             d_flags, (hipStream_t)stream);                                                     \
  }
SH_LSAP_ENTRIES(i64, int64_t, int64_t, int64_t, solve_i64)
SH_LSAP_ENTRIES(i32, int32_t, int32_t, int64_t, solve_i64)
SH_LSAP_ENTRIES(f64, double, double, double, solve_f64)
SH_LSAP_ENTRIES(f32, float, float, double, solve_f64)
SH_LSAP_ENTRIES(f16, uint16_t, _Float16, double, solve_f64)
SH_LSAP_ENTRIES(bf16, uint16_t, sh_bf16, double, solve_f64)
#undef SH_LSAP_ENTRIES

// The warm-start entry of a dense cost type (launch_warm): d_col and d_v are
// in / out, d_u out, d_cost and d_kept nullable.
#define SH_WARM_ENTRY(SUF, CT, KT, T)                                                                          \
  int lsap_warm_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape, int32_t *d_col, T *d_cost, \
                      T *d_u, T *d_v, int32_t *d_kept, unsigned flags, void *stream) {                         \
    return launch_warm((const KT *)d_C, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, d_kept, flags,            \
                       (hipStream_t)stream);                                                                   \
  }
SH_WARM_ENTRY(i64, int64_t, int64_t, int64_t)
SH_WARM_ENTRY(i32, int32_t, int32_t, int64_t)
SH_WARM_ENTRY(f64, double, double, double)
SH_WARM_ENTRY(f32, float, float, double)
SH_WARM_ENTRY(f16, uint16_t, _Float16, double)
SH_WARM_ENTRY(bf16, uint16_t, sh_bf16, double)
#undef SH_WARM_ENTRY

// ... and with free rows (launch_warm_fr): d_kept [B x 2] and d_theta [B] are
// out and nullable.
#define SH_WARM_FR_ENTRY(SUF, CT, KT, T)                                                                       \
  int lsap_warm_fr_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape, int32_t *d_col,         \
                         T *d_cost, T *d_u, T *d_v, int32_t *d_kept, T *d_theta, unsigned flags,               \
                         void *stream) {                                                                       \
    return launch_warm_fr((const KT *)d_C, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, d_kept, d_theta,       \
                          flags, (hipStream_t)stream);                                                         \
  }
SH_WARM_FR_ENTRY(i64, int64_t, int64_t, int64_t)
SH_WARM_FR_ENTRY(i32, int32_t, int32_t, int64_t)
SH_WARM_FR_ENTRY(f64, double, double, double)
SH_WARM_FR_ENTRY(f32, float, float, double)
SH_WARM_FR_ENTRY(f16, uint16_t, _Float16, double)
SH_WARM_FR_ENTRY(bf16, uint16_t, sh_bf16, double)
#undef SH_WARM_FR_ENTRY

// The k-best entries of a float cost type (murty_children, kbest); FR: with free rows.
#define SH_KBEST_ENTRIES(NAME, CT, FR)                                                                          \
  int lsap_murty_children_##NAME(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape,                  \
                                 const int32_t *d_pcol, const double *d_pv, const int32_t *d_p,                 \
                                 const uint64_t *d_forb, int32_t *d_col, double *d_cost, double *d_u,           \
                                 double *d_v, int32_t *d_kept, unsigned flags, void *stream) {                  \
    (void)flags;                                                                                                \
    return murty_children(d_C, nr, nc, B, d_shape, d_pcol, d_pv, d_p, d_forb, d_col, d_cost, d_u, d_v, d_kept,  \
                          FR, (hipStream_t)stream);                                                             \
  }                                                                                                             \
  int lsap_kbest_##NAME(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape, int k, int32_t *d_cols,   \
                        double *d_costs, int32_t *d_count, void *d_work, size_t work_bytes, unsigned flags,     \
                        void *stream) {                                                                         \
    return kbest(d_C, nr, nc, B, d_shape, k, d_cols, d_costs, d_count, d_work, work_bytes, flags, FR,           \
                 (hipStream_t)stream);                                                                          \
  }
SH_KBEST_ENTRIES(f64, double, false)
SH_KBEST_ENTRIES(f32, float, false)
SH_KBEST_ENTRIES(fr_f64, double, true)
SH_KBEST_ENTRIES(fr_f32, float, true)
#undef SH_KBEST_ENTRIES

size_t lsap_kbest_work_bytes(int nr, int nc, int B, int k) {
  if (nr < 1 || nr > nc || nc > SH_MAX_N || B < 0 || k < 1 || (uint64_t)B * (uint64_t)nr > (uint64_t)INT32_MAX)
    return 0;
  return kbest_carve(nullptr, nr, nc, B, k, nullptr);
}

int lsap_solve_batched_rect_hash(uint64_t seed, int64_t modulus, int nr, int nc, int B,
                                 int32_t *d_col, int64_t *d_cost, unsigned flags, void *stream) {
  if (modulus <= 0) return fail(SH_ERR_ARGS, "modulus must be > 0");
  HIP_TRY_RC(check_lsap_args(nr, nc, B, d_col, SH_MAX_N));
  return launch_i64<int64_t, true>(nullptr, seed, modulus, nr, nc, B, nullptr, d_col, d_cost, nullptr, nullptr,
                                   flags, (hipStream_t)stream);
}

size_t lsap_csr_work_bytes(int nr, int nc, int B) {
  if (nr < 1 || nc < 1 || B < 1) return 0;
  return (csr_words(nr, nc, B) * (sizeof(uint64_t) + sizeof(uint16_t)) + 15) / 16 * 16;
}

int lsap_solve_csr_f64(const int64_t *d_indptr, const int32_t *d_indices, const double *d_data, int nr, int nc,
                       int B, const int32_t *d_shape, int32_t *d_col, double *d_cost, double *d_u, double *d_v,
                       void *d_work, size_t work_bytes, unsigned flags, void *stream) {
  return launch_lsap_csr(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, d_work,
                         work_bytes, flags, (hipStream_t)stream);
}

int lsap_solve_csr_f32(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, int nr, int nc,
                       int B, const int32_t *d_shape, int32_t *d_col, double *d_cost, double *d_u, double *d_v,
                       void *d_work, size_t work_bytes, unsigned flags, void *stream) {
  return launch_lsap_csr(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, d_work,
                         work_bytes, flags, (hipStream_t)stream);
}

// The warm-start entry of a CSR value type (launch_warm_csr): d_col and d_v are
// in / out, d_u out, d_cost and d_kept nullable.
#define SH_WARM_CSR_ENTRY(SUF, CT)                                                                              \
  int lsap_warm_csr_##SUF(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr, int nc,  \
                          int B, const int32_t *d_shape, int32_t *d_col, double *d_cost, double *d_u,           \
                          double *d_v, int32_t *d_kept, void *d_work, size_t work_bytes, unsigned flags,        \
                          void *stream) {                                                                       \
    return launch_warm_csr(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, d_kept,    \
                           d_work, work_bytes, flags, (hipStream_t)stream);                                     \
  }
SH_WARM_CSR_ENTRY(f64, double)
SH_WARM_CSR_ENTRY(f32, float)
#undef SH_WARM_CSR_ENTRY

// ... and with free rows (launch_warm_fr_csr): d_kept [B x 2] and d_theta [B]
// are out and nullable.
#define SH_WARM_FR_CSR_ENTRY(SUF, CT)                                                                             \
  int lsap_warm_fr_csr_##SUF(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr, int nc, \
                             int B, const int32_t *d_shape, int32_t *d_col, double *d_cost, double *d_u,          \
                             double *d_v, int32_t *d_kept, double *d_theta, void *d_work, size_t work_bytes,      \
                             unsigned flags, void *stream) {                                                      \
    return launch_warm_fr_csr(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_col, d_cost, d_u, d_v, d_kept,   \
                              d_theta, d_work, work_bytes, flags, (hipStream_t)stream);                           \
  }
SH_WARM_FR_CSR_ENTRY(f64, double)
SH_WARM_FR_CSR_ENTRY(f32, float)
#undef SH_WARM_FR_CSR_ENTRY

// The k-best entries of a CSR value type (murty_children_csr, kbest_csr); FR: with free rows.
#define SH_KBEST_CSR_ENTRIES(NAME, CT, FR)                                                                         \
  int lsap_murty_children_##NAME(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr,      \
                                 int nc, int B, const int32_t *d_shape, const int32_t *d_pcol,                     \
                                 const double *d_pv, const int32_t *d_p, const uint64_t *d_forb,                   \
                                 int32_t *d_col, double *d_cost, double *d_u, double *d_v, int32_t *d_kept,        \
                                 void *d_work, size_t work_bytes, unsigned flags, void *stream) {                  \
    (void)flags;                                                                                                   \
    return murty_children_csr(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_pcol, d_pv, d_p, d_forb, d_col,   \
                              d_cost, d_u, d_v, d_kept, d_work, work_bytes, FR, (hipStream_t)stream);              \
  }                                                                                                                \
  int lsap_kbest_##NAME(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr, int nc,       \
                        int B, const int32_t *d_shape, int k, int32_t *d_cols, double *d_costs,                    \
                        int32_t *d_count, void *d_work, size_t work_bytes, unsigned flags, void *stream) {         \
    return kbest_csr(d_indptr, d_indices, d_data, nr, nc, B, d_shape, k, d_cols, d_costs, d_count, d_work,         \
                     work_bytes, flags, FR, (hipStream_t)stream);                                                  \
  }
SH_KBEST_CSR_ENTRIES(csr_f64, double, false)
SH_KBEST_CSR_ENTRIES(csr_f32, float, false)
SH_KBEST_CSR_ENTRIES(fr_csr_f64, double, true)
SH_KBEST_CSR_ENTRIES(fr_csr_f32, float, true)
#undef SH_KBEST_CSR_ENTRIES

size_t lsap_kbest_csr_work_bytes(int nr, int nc, int B, int k) {
  if (nr < 1 || nr > nc || nc > SH_MAX_N || B < 0 || k < 1 || (uint64_t)B * (uint64_t)nr > (uint64_t)INT32_MAX)
    return 0;
  return kbest_csr_bytes(nr, nc, B, k, nullptr);
}

// The certificates of a CSR value type (launch_csr_cert, launch_csr_match,
// launch_csr_hall_check).  The matching takes no launch-forcing flag: it has
// one configuration, and `flags` is not read.
#define SH_CSR_CERT_ENTRIES(SUF, CT)                                                                             \
  int lsap_check_duals_csr_##SUF(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr,    \
                                 int nc, int B, const int32_t *d_shape, const int32_t *d_col, const double *d_u, \
                                 const double *d_v, double *d_slack, int32_t *d_flags, void *stream) {           \
    return launch_csr_cert(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_col, d_u, d_v, d_slack, d_flags,   \
                           (hipStream_t)stream);                                                                 \
  }                                                                                                              \
  int lsap_match_csr_##SUF(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr, int nc,  \
                           int B, const int32_t *d_shape, int32_t *d_match, int32_t *d_card, uint8_t *d_wit,     \
                           void *d_work, size_t work_bytes, unsigned flags, void *stream) {                      \
    (void)flags;                                                                                                 \
    return launch_csr_match(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_match, d_card, d_wit, d_work,     \
                            work_bytes, (hipStream_t)stream);                                                    \
  }                                                                                                              \
  int lsap_check_hall_csr_##SUF(const int64_t *d_indptr, const int32_t *d_indices, const CT *d_data, int nr,     \
                                int nc, int B, const int32_t *d_shape, const int32_t *d_match,                   \
                                const uint8_t *d_wit, int32_t *d_counts, int32_t *d_flags, void *stream) {       \
    return launch_csr_hall_check(d_indptr, d_indices, d_data, nr, nc, B, d_shape, d_match, d_wit, d_counts,      \
                                 d_flags, (hipStream_t)stream);                                                  \
  }
SH_CSR_CERT_ENTRIES(f64, double)
SH_CSR_CERT_ENTRIES(f32, float)
#undef SH_CSR_CERT_ENTRIES

#define SH_LBAP_ENTRY(SUF, CT, DT)                                                                       \
  int lbap_solve_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape, int32_t *d_col,     \
                       CT *d_value, unsigned flags, void *stream) {                                      \
    return launch_lbap<DT>(d_C, nr, nc, B, d_shape, d_col, d_value, flags, (hipStream_t)stream);         \
  }                                                                                                      \
  int lbap_solve_wit_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape, int32_t *d_col, \
                           CT *d_value, uint8_t *d_wit, unsigned flags, void *stream) {                  \
    return launch_lbap<DT, true>(d_C, nr, nc, B, d_shape, d_col, d_value, flags, (hipStream_t)stream,    \
                                 d_wit);                                                                 \
  }                                                                                                      \
  int lbap_check_##SUF(const CT *d_C, int nr, int nc, int B, const int32_t *d_shape,                     \
                       const int32_t *d_col, const CT *d_value, const uint8_t *d_wit, int32_t *d_counts, \
                       int32_t *d_flags, unsigned flags, void *stream) {                                 \
    return launch_lbap_check<DT>(d_C, nr, nc, B, d_shape, d_col, d_value, d_wit, d_counts, d_flags,      \
                                 flags, (hipStream_t)stream);                                            \
  }
SH_LBAP_ENTRY(i64, int64_t, LBAP_I64)
SH_LBAP_ENTRY(i32, int32_t, LBAP_I32)
SH_LBAP_ENTRY(f64, double, LBAP_F64)
SH_LBAP_ENTRY(f32, float, LBAP_F32)
SH_LBAP_ENTRY(f16, uint16_t, LBAP_F16)
SH_LBAP_ENTRY(bf16, uint16_t, LBAP_BF16)
#undef SH_LBAP_ENTRY

// The square entries: nr == nc == n, no shapes.
int lsap_solve_batched_i64(const int64_t *d_C, int n, int B, int32_t *d_col, int64_t *d_cost,
                           unsigned flags, void *stream) {
  return lsap_solve_batched_rect_i64(d_C, n, n, B, nullptr, d_col, d_cost, flags, stream);
}

int lsap_solve_batched_i32(const int32_t *d_C, int n, int B, int32_t *d_col, int64_t *d_cost,
                           unsigned flags, void *stream) {
  return lsap_solve_batched_rect_i32(d_C, n, n, B, nullptr, d_col, d_cost, flags, stream);
}

int lsap_solve_batched_f64(const double *d_C, int n, int B, int32_t *d_col, double *d_cost,
                           unsigned flags, void *stream) {
  return lsap_solve_batched_rect_f64(d_C, n, n, B, nullptr, d_col, d_cost, flags, stream);
}

int lsap_solve_batched_hash(uint64_t seed, int64_t modulus, int n, int B, int32_t *d_col,
                            int64_t *d_cost, unsigned flags, void *stream) {
  return lsap_solve_batched_rect_hash(seed, modulus, n, n, B, d_col, d_cost, flags, stream);
}

}  // extern "C"

