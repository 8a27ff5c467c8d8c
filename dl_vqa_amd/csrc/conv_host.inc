// Host-side scaffolding shared by conv.hip, conv_bf16.hip and conv_x3.hip (included inside namespace vqa, after
// conv_device.inc): geometry checks, the batch-chunk walk, the split-K plan and workspace layout of wgrad.  The generic launch
// helpers (launch_kernel, with_flag) are in common.hpp.
// a kernel with one workgroup per tile and its persistent twin take the same arguments; only the grid differs
template <class KP, class K, class... A>
static int launch_tiles(bool persistent, KP pkern, KernelNames pn, int pgrid, K kern, KernelNames n, int grid, int threads,
                        int lds, hipStream_t s, A... args) {
  return persistent ? launch_kernel(pkern, pn, pgrid, threads, lds, s, args...)
                    : launch_kernel(kern, n, grid, threads, lds, s, args...);
}

static int check_geom(const char* fn, const ConvGeom& g) {
  VQA_REQUIRE(g.B > 0 && g.H >= 3 && g.W >= 3, "%s: bad image shape B=%d H=%d W=%d", fn, g.B, g.H, g.W);
  VQA_REQUIRE(g.CiP % 4 == 0 && g.Co % 4 == 0 && g.CiP > 0 && g.Co > 0,
              "%s: channel counts must be positive multiples of 4 (CiP=%d Co=%d)", fn, g.CiP, g.Co);
  VQA_REQUIRE(g.stride == 1 || g.stride == 2, "%s: stride %d unsupported (1 or 2)", fn, g.stride);
  VQA_REQUIRE(g.Hp > 0 && g.Wp > 0, "%s: image too small for conv+pool", fn);
  VQA_REQUIRE((int64_t)g.B * g.H * g.W < (1LL << 31) / 4, "%s: too many pixels for 32-bit row indices", fn);
  // the loaders address each tensor with 32-bit byte offsets from its first element
  VQA_REQUIRE((int64_t)g.B * g.H * g.W * g.CiP * 4 < 0xffff0000LL && (int64_t)g.B * g.Hp * g.Wp * g.Co * 4 < 0xffff0000LL,
              "%s: a tensor of this launch reaches 4 GiB (B=%d)", fn, g.B);
  return VQA_OK;
}

// The loaders address every tensor with 32-bit byte offsets, so a launch covers at most `chunk` images (all
// tensors of the layer below 4 GiB, pixel rows below 2^29); the C ABI entry points walk larger batches in
// chunks -- images are independent, wgrad's chunks are simply more split-K slabs for the same reduce.
static int batch_chunk(int B, int H, int W, int CiP, int Co, int stride) {
  const ConvGeom g = make_geom(1, H, W, CiP, Co, stride);
  const int64_t in_b = (int64_t)H * W * CiP * 4, out_b = (int64_t)(g.Hp > 0 ? g.Hp : 1) * (g.Wp > 0 ? g.Wp : 1) * Co * 4;
  const int64_t per_img = in_b > out_b ? in_b : out_b;
  int64_t c = (0xffff0000LL - 1) / per_img;
  const int64_t by_rows = ((1LL << 31) / 4 - 1) / ((int64_t)H * W);
  if (by_rows < c) c = by_rows;
  if (c > B) c = B;
  {   // tests: force small chunks on small tensors (VQA_CONV_CHUNK)
    const int64_t f = knobs().conv_chunk;
    if (f > 0 && f < c) c = f;
  }
  return (int)c;     // 0: a single image is already too large
}

// ---- the chunk walk
// One call of an entry point `fn`: the layer, the batch and the images per launch (batch_chunk, or the family's own rule).
struct ConvWalk { const char* fn; int B, H, W, CiP, Co, stride, chunk; };
// One launch of the walk: its geometry and the ELEMENT offsets of its first image in the input-side (xo: [H][W][CiP])
// and pooled-side (po: [Hp][Wp][Co]) tensors; the caller scales them by its own element sizes.
struct ConvChunk { int b0; ConvGeom g; int64_t xo, po; };

static bool no_windows(int B, int H, int W, int stride) {
  const ConvGeom g1 = make_geom(1, H, W, 4, 4, stride);
  return B <= 0 || g1.Hp <= 0 || g1.Wp <= 0;
}

template <class F>
static int walk_chunks(const ConvWalk& w, F&& body) {
  const ConvGeom g1 = make_geom(1, w.H, w.W, w.CiP, w.Co, w.stride);
  for (int b0 = 0; b0 < w.B; b0 += w.chunk) {
    const ConvGeom g = make_geom(w.B - b0 < w.chunk ? w.B - b0 : w.chunk, w.H, w.W, w.CiP, w.Co, w.stride);
    int rc = check_geom(w.fn, g);
    if (rc) return rc;
    rc = body(ConvChunk{b0, g, (int64_t)b0 * w.H * w.W * w.CiP, (int64_t)b0 * g1.Hp * g1.Wp * w.Co});
    if (rc) return rc;
  }
  return VQA_OK;
}

// forward / dgrad entry points: body(chunk) chooses the tile and launches
template <class F>
static int for_each_chunk(const ConvWalk& w, int kernel_id, int tag, hipStream_t s, F&& body) {
  VQA_REQUIRE(w.chunk > 0, "%s: one %dx%dx%d image reaches 4 GiB", w.fn, w.H, w.W, w.CiP);
  set_launch_tag(tag);
  ProfScope prof(kernel_id, s);
  return walk_chunks(w, body);
}

// ---- wgrad: split-K over the conv-output pixels into slabs [KI = 9*CiP][Co], then one reduce
// bias_parts: partial bias rows [Co] the launch writes next to its slabs (0: the family sums the bias elsewhere)
struct WgradPlan { int tiles_m, tiles_n, nk, splits, ks_per_split, Mtot, KI, bias_parts; };
// bm x bn tiles, K-steps of `kstep` pixels, split so that tiles * splits fills but does not exceed `slots` resident
// workgroups, with at least 8 K-steps per split
static WgradPlan plan_splits(const ConvGeom& g, int bm, int bn, int kstep, int slots) {
  WgradPlan p{};
  p.KI = 9 * g.CiP;
  p.Mtot = g.B * 2 * g.Hp * 2 * g.Wp;
  p.tiles_m = (p.KI + bm - 1) / bm;
  p.tiles_n = (g.Co + bn - 1) / bn;
  p.nk = (p.Mtot + kstep - 1) / kstep;
  int splits = slots / (p.tiles_m * p.tiles_n);
  if (splits < 1) splits = 1;
  const int max_splits = p.nk / 8 > 1 ? p.nk / 8 : 1;
  if (splits > max_splits) splits = max_splits;
  p.ks_per_split = (p.nk + splits - 1) / splits;
  p.splits = (p.nk + p.ks_per_split - 1) / p.ks_per_split;
  return p;
}

// Slabs and bias rows of a whole batch.  *_workspace_bytes and *_wgrad both take the workspace layout from here:
// all slabs first, in chunk order, then all bias rows.
struct SlabCount { int64_t splits, bias_parts; };
template <class P>
static SlabCount count_slabs(const ConvWalk& w, P plan) {
  SlabCount n{0, 0};
  if (w.chunk <= 0 || no_windows(w.B, w.H, w.W, w.stride)) return n;
  for (int b0 = 0; b0 < w.B; b0 += w.chunk) {
    const auto p = plan(make_geom(w.B - b0 < w.chunk ? w.B - b0 : w.chunk, w.H, w.W, w.CiP, w.Co, w.stride));
    n.splits += p.splits;
    n.bias_parts += p.bias_parts;
  }
  return n;
}
static int64_t slab_bytes(const ConvWalk& w, SlabCount n) {
  return (n.splits * 9 * w.CiP * w.Co + n.bias_parts * w.Co) * 4;
}

static int reduce_bias_rows(const float* rows, float* dbias, int n, int Co, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_bias_reduce_kernel, dim3((Co + 31) / 32), dim3(256), 0, s, rows, dbias, n, Co);
  return check_hip(hipGetLastError(), "wgrad_bias_reduce launch");
}

// wgrad entry points: workspace check, body(chunk, plan(chunk.g), slab, bias_rows) per chunk, the reduce into dw, then
// bias_tail(first bias row, rows) -- all inside one ProfScope.  extra_bytes: workspace the family keeps after the bias rows.
template <class P, class F, class T>
static int wgrad_walk(const ConvWalk& w, P plan, int64_t extra_bytes, float* workspace, int64_t workspace_bytes, float* dw,
                      int Ci, int tag, hipStream_t s, F&& body, T&& bias_tail) {
  VQA_REQUIRE(w.chunk > 0, "%s: one %dx%dx%d image reaches 4 GiB", w.fn, w.H, w.W, w.CiP);
  const SlabCount n = count_slabs(w, plan);
  const int64_t need = n.splits ? slab_bytes(w, n) + extra_bytes : 0;
  if (workspace_bytes < need) {
    set_error("%s: workspace %lld < %lld", w.fn, (long long)workspace_bytes, (long long)need);
    return VQA_ERR_WORKSPACE;
  }
  const int64_t slab = (int64_t)9 * w.CiP * w.Co;
  float* const bias0 = workspace + n.splits * slab;
  set_launch_tag(tag);
  ProfScope prof(VQA_K_CONV_WGRAD, s);
  int64_t done = 0, bdone = 0;
  int rc = walk_chunks(w, [&](const ConvChunk& c) {
    const auto p = plan(c.g);
    const int r = body(c, p, workspace + done * slab, bias0 + bdone * w.Co);
    done += p.splits;
    bdone += p.bias_parts;
    return r;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((9 * w.CiP * w.Co + 63) / 64), dim3(256), 0, s, workspace, dw,
                     (int)n.splits, 9 * w.CiP, w.CiP, Ci, w.Co);
  rc = check_hip(hipGetLastError(), "wgrad_reduce launch");
  if (rc) return rc;
  return bias_tail(bias0, (int)n.bias_parts);
}
