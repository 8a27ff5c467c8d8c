// Device side of conv.hip (loaders, kernels). Included once by conv.hip.
#ifdef VQA_EXP_NOAM   // timing experiment: skip the arg-max loads
#define AM_LOAD(...) 0u
#else
#define AM_LOAD(...) buf_load4(__VA_ARGS__)
#endif

struct ConvGeom {
  int B, H, W, CiP, Co, stride, Ho, Wo, Hp, Wp;
};
static ConvGeom make_geom(int B, int H, int W, int CiP, int Co, int stride) {
  ConvGeom g{B, H, W, CiP, Co, stride, 0, 0, 0, 0};
  g.Ho = (H - 3) / stride + 1;
  g.Wo = (W - 3) / stride + 1;
  g.Hp = g.Ho / 2;
  g.Wp = g.Wo / 2;
  return g;
}

// K index of the convolution GEMMs is (tap = ky*3+kx, channel); a K-step advances by BK channels, carried
// incrementally (no integer division in the K loop).  When the channel count is a multiple of BK a K-step
// lies inside one tap, the cursor starts at a uniform k and lives in SGPRs; otherwise every 16-byte chunk
// has its own tap and the cursor is per lane.
struct TapCursor {
  int tap, ch, C;
  __device__ __forceinline__ void init(int k, int C_) { C = C_; tap = k / C_; ch = k - tap * C_; }
  __device__ __forceinline__ void advance() {
    ch += BK;
    while (ch >= C) { ch -= C; ++tap; }
  }
};

// All activation tensors are addressed with 32-bit byte offsets from the tensor's first element
// (check_geom: every tensor of a layer is below 4 GiB).

// ------------------------------------------------------------------ forward A loader (type R)
// UT (uniform tap): CiP % BK == 0, a K-step lies inside one tap: the cursor is scalar, the tap / channel
// offset goes into the buffer base and the K loop has no VALU instruction.  Otherwise every 16-byte chunk
// has its own tap (per-lane cursor; the general path for small or odd channel counts).
template <int NV, int LT, bool UT>
struct ConvFwdA {
  struct Params { const float* x; int H, W, CiP, Hp, Wp, stride, nWin, K; };
  struct Raw { float4 v[NV]; };
  static constexpr bool kTypeR = true;
  const float* x;
  uint32_t voff[NV];      // byte offset of (pixel of row p, channel 4*chunk if UT); BUF_OOB for rows past the end
  int W, CiP;
  TapCursor cur;
  __device__ __forceinline__ void init(const Params& q, int row0, int tid, int ks0) {
    x = q.x; W = q.W; CiP = q.CiP;
    const int c4 = 4 * StageMap<LT>::r_chunk(tid);
    cur.init(ks0 * BK + (UT ? 0 : c4), q.CiP);
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int m = row0 + StageMap<LT>::r_row(tid, p);
      const int wl = m >> 2, j = m & 3;
      const int px = wl % q.Wp;
      const int t = wl / q.Wp;
      const int py = t % q.Hp;
      const int b = t / q.Hp;
      const int y = (2 * py + (j >> 1)) * q.stride, xx = (2 * px + (j & 1)) * q.stride;
      const uint32_t e = (uint32_t)((b * q.H + y) * q.W + xx) * (uint32_t)q.CiP + (UT ? (uint32_t)c4 : 0u);
      voff[p] = wl < q.nWin ? e * 4u : BUF_OOB;
    }
  }
  __device__ __forceinline__ void issue(int /*ks*/, Raw& r) {
    const bool kok = cur.tap < 9;
    const int tap = kok ? cur.tap : 0;
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int koff = (ky * W + kx) * CiP + cur.ch;
    if (UT) {
      // past the last tap the resource is empty: every lane reads zeros
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(x + koff, kok ? BUF_OOB : 0u);
#pragma unroll
      for (int p = 0; p < NV; ++p) r.v[p] = buf_load16(rs, voff[p]);
    } else {
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(x);
#pragma unroll
      for (int p = 0; p < NV; ++p)
        r.v[p] = buf_load16(rs, kok && voff[p] != BUF_OOB ? voff[p] + 4u * (uint32_t)koff : BUF_OOB);
    }
    cur.advance();
  }
  __device__ __forceinline__ void finish(const Raw& r, float4 (&o)[NV]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) o[p] = r.v[p];
  }
};

// bias + ReLU + 2x2 max-pool + arg-max on the accumulators of one tile (register only).  Row order
// m = 4*window + j puts a window's four pixels into four consecutive accumulator registers of one lane.
// Stores go through buffer resources based at the 32x32 tile's first window / column: the lane's part
// (window lane>>5, column lane&31) is one VGPR, group g's two windows a scalar offset; on edge tiles an
// invalid element's offset is BUF_OOB and the store is dropped.
// OB: the pooled activation is stored as bf16 (2-byte elements; the bf16 path), otherwise fp32.
template <class Cfg, bool OB = false>
__device__ __forceinline__ void conv_pool_epilogue(f32x16 (&acc)[Cfg::TM][Cfg::TN], const float* __restrict__ bias,
                                                   void* pooled_, uint8_t* amax, int nWin, int Co, int m0, int n0,
                                                   int wm, int wn, int lane) {
  float* pooled = static_cast<float*>(pooled_);
  uint16_t* pooled16 = static_cast<uint16_t*>(pooled_);
  const int h = lane >> 5;
  const bool interior = (m0 + Cfg::BM) / 4 <= nWin && n0 + Cfg::BN <= Co;   // uniform
  const uint32_t vl = (uint32_t)(h * Co + (lane & 31));                     // elements; x4 for pooled, x1 for amax
  auto body = [&](auto inner) {
    constexpr bool INNER = decltype(inner)::value;
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const int colt = n0 + wn * Cfg::WN + 32 * j;
      const int col = colt + (lane & 31);
      const float bv = INNER || col < Co ? bias[INNER || col < Co ? col : 0] : 0.f;
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i) {
        const int wt = (m0 + wm * Cfg::WM + 32 * i) >> 2;                   // tile's first window (uniform)
        const int64_t o0 = (int64_t)wt * Co + colt;
        const __amdgpu_buffer_rsrc_t rp = OB ? buf_rsrc(pooled16 + o0) : buf_rsrc(pooled + o0), ra = buf_rsrc(amax + o0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const PoolPick p = pool_pick(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], bv);
          const bool ok = INNER || (wt + 2 * g + h < nWin && col < Co);
          const uint32_t so = (uint32_t)(2 * g * Co);
#ifdef VQA_EXP_NOSTORE_ALL   // timing experiments only: the epilogue's arithmetic without its store instructions
          if (Co < 0)
#endif
          {
          if (OB) buf_store2(rp, bf16_bits(p.v), ok ? 2u * vl : BUF_OOB, 2u * so);
          else buf_store4(rp, p.v, ok ? 4u * vl : BUF_OOB, 4u * so);
          }
#if defined(VQA_EXP_NOSTORE_ALL) || defined(VQA_EXP_NOSTORE_AM)
          if (Co < 0)
#endif
          buf_store1(ra, p.code, ok ? vl : BUF_OOB, so);
        }
      }
    }
  };
  if (interior) body(std::true_type{}); else body(std::false_type{});
}

// The same epilogue with 16-byte stores through LDS, for interior 128x128 tiles of the one-workgroup-per-tile kernel (fp32
// output, Co % 16 == 0).  The direct form issues 32 store instructions per wave and tile -- 16 dword stores of two 128-byte
// runs and 16 BYTE stores of two 32-byte runs -- and the store issue rate, not the bytes, is what they cost: without the
// arg-max stores conv1 forward ran 3.30 -> 3.20 ms, without any store 3.13 ms (B = 256; tools/probe_conv_fwd.py with
// -DVQA_EXP_NOSTORE_AM / _ALL builds).  Here a wave writes its 16 windows x 64 channels of pooled values (4 KB) and arg-max
// bytes (1 KB) into a wave-private scratch -- the stage buffers are free: the last K-step barrier has passed, the loader
// waves have exited and every MFMA wave holds its last fragments in registers -- and stores them as 4 + 1 instructions of
// 16 bytes per lane: a window's 64 channels are one 256-byte run of pooled and one 64-byte run of arg-max.  Same values.
template <class Cfg>
__device__ __forceinline__ void conv_pool_epilogue_staged(f32x16 (&acc)[Cfg::TM][Cfg::TN], const float* __restrict__ bias,
                                                          float* pooled, uint8_t* amax, int Co, int m0, int n0, int wm,
                                                          int wn, int lane, float* smem) {
  static_assert(Cfg::WM == 64 && Cfg::WN == 64 && Cfg::TM == 2 && Cfg::TN == 2, "64 x 64 wave blocks");
  constexpr int SCR = 4096 + 1024;                                       // bytes per wave: pooled [16][64] f32, arg-max [16][64] u8
  char* const scr = reinterpret_cast<char*>(smem) + (wm * Cfg::WAVES_N + wn) * SCR;
  float* const sp = reinterpret_cast<float*>(scr);
  uint8_t* const sa = reinterpret_cast<uint8_t*>(scr + 4096);
  const int h = lane >> 5, c = lane & 31;
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j) {
    const float bv = bias[n0 + wn * Cfg::WN + 32 * j + c];
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const PoolPick p = pool_pick(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], bv);
        const int w = 8 * i + 2 * g + h;                                 // window of the wave's 16 (rows 32i + 8g + 4h ..+3)
        sp[w * 64 + 32 * j + c] = p.v;
        sa[w * 64 + 32 * j + c] = p.code;
      }
    }
  }
  asm volatile("" ::: "memory");     // the wave's LDS accesses execute in order; keep the compiler's order as well
  const int64_t o0 = (int64_t)((m0 + wm * Cfg::WM) >> 2) * Co + n0 + wn * Cfg::WN;   // first window, first channel of the wave
  const __amdgpu_buffer_rsrc_t rp = buf_rsrc(pooled + o0), ra = buf_rsrc(amax + o0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = q * 64 + lane;                                       // 16-byte piece: window idx / 16, channels 4 * (idx % 16)
    const float4 v = *reinterpret_cast<const float4*>(scr + idx * 16);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rp,
                                           (int)(((uint32_t)(idx >> 4) * (uint32_t)Co + 4u * (uint32_t)(idx & 15)) * 4u), 0, 0);
  }
  {
    const float4 v = *reinterpret_cast<const float4*>(scr + 4096 + lane * 16);    // window lane / 4, channels 16 * (lane % 4)
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ra,
                                           (int)((uint32_t)(lane >> 2) * (uint32_t)Co + 16u * (uint32_t)(lane & 3)), 0, 0);
  }
}

template <class Cfg, bool U>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void conv_fwd_kernel(typename ConvFwdA<Cfg::NVA, Cfg::LT, U>::Params pa,
                                                       typename PlainC<Cfg::NVB, Cfg::LT>::Params pb,
                                                       const float* __restrict__ bias, float* pooled,
                                                       uint8_t* amax, int Co, int tiles_m, int tiles_n, int nk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  const TileCoord tc = tile_coord(tiles_m, tiles_n);
  const int m0 = tc.mt * Cfg::BM, n0 = tc.nt * Cfg::BN;
  using AL = ConvFwdA<Cfg::NVA, Cfg::LT, U>;
  using BL = PlainC<Cfg::NVB, Cfg::LT>;
  f32x16 acc[Cfg::TM][Cfg::TN];
  acc_zero<Cfg>(acc);
  if (!gemm_mainloop<Cfg, AL, BL, (Cfg::BN <= 64)>(
          [&](AL& al, BL& bl) {
            al.init(pa, m0, loader_tid<Cfg>(), 0);
            bl.init(pb, n0, loader_tid<Cfg>(), 0);
          },
          [](AL&, BL&) {}, acc, 0, nk, pa.K, smem))
    return;
#ifndef VQA_EXP_NO_STAGED_POOL   // A/B builds of the direct epilogue (tools/build_variant.sh)
  if constexpr (Cfg::WM == 64 && Cfg::WN == 64 && Cfg::TM == 2 && Cfg::TN == 2) {
    // interior tile, 16-byte aligned rows: the wide-store form (uniform test)
    if ((m0 + Cfg::BM) / 4 <= pa.nWin && n0 + Cfg::BN <= Co && (Co & 15) == 0 &&
        ((reinterpret_cast<uintptr_t>(pooled) | reinterpret_cast<uintptr_t>(amax)) & 15) == 0)
      return conv_pool_epilogue_staged<Cfg>(acc, bias, pooled, amax, Co, m0, n0, wm, wn, lane, smem);
  }
#endif
  conv_pool_epilogue<Cfg>(acc, bias, pooled, amax, pa.nWin, Co, m0, n0, wm, wn, lane);
}

// persistent variant: a resident set of workgroups walks the tiles (gemm_persistent)
template <class Cfg, bool U>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void conv_fwd_persistent_kernel(
    typename ConvFwdA<Cfg::NVA, Cfg::LT, U>::Params pa, typename PlainC<Cfg::NVB, Cfg::LT>::Params pb, const float* __restrict__ bias,
    float* pooled, uint8_t* amax, int Co, int tiles_m, int tiles_n, int nk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  using AL = ConvFwdA<Cfg::NVA, Cfg::LT, U>;
  using BL = PlainC<Cfg::NVB, Cfg::LT>;
  gemm_persistent<Cfg, AL, BL, (Cfg::BN <= 64)>(
      xcd_swizzle(blockIdx.x, gridDim.x), gridDim.x, tiles_m * tiles_n, nk, pa.K, smem,
      [&](int t, AL& al, BL& bl) {
        const int mt = t / tiles_n, nt = t - mt * tiles_n;
        al.init(pa, mt * Cfg::BM, loader_tid<Cfg>(), 0);
        bl.init(pb, nt * Cfg::BN, loader_tid<Cfg>(), 0);
      },
      [&](int t, f32x16 (&acc)[Cfg::TM][Cfg::TN]) {
        const int mt = t / tiles_n, nt = t - mt * tiles_n;
        conv_pool_epilogue<Cfg>(acc, bias, pooled, amax, pa.nWin, Co, mt * Cfg::BM, nt * Cfg::BN, wm, wn, lane);
      });
}

// ------------------------------------------------------------------ pooled-gradient expansion
// dY(pixel) = dP(window) where the stored arg-max byte equals the pixel's position j in its window.
// id holds the arg-max bytes of the chunk's four channels, j is the pixel's position in its window (a dead
// window stores 4, which matches no j).  Two VALU instructions per element: a byte-select (SDWA) compare
// into an SGPR pair and the select on it; the four compares precede the four selects, which also covers
// the two wait states gfx950 wants between a VALU write of an SGPR and its use as a lane mask.
__device__ __forceinline__ float4 route4(float4 d, uint32_t id, uint32_t j) {
#ifdef VQA_EXP_NOROUTE   // timing experiments only (tools/build_variant.sh): what the routing VALU costs
  d.x += __uint_as_float((id + j) & 0u);
  return d;
#endif
  float4 r;
  unsigned long long m0, m1, m2, m3;
  asm("v_cmp_eq_u32_sdwa %4, %8, %9 src0_sel:BYTE_0 src1_sel:DWORD\n\t"
      "v_cmp_eq_u32_sdwa %5, %8, %9 src0_sel:BYTE_1 src1_sel:DWORD\n\t"
      "v_cmp_eq_u32_sdwa %6, %8, %9 src0_sel:BYTE_2 src1_sel:DWORD\n\t"
      "v_cmp_eq_u32_sdwa %7, %8, %9 src0_sel:BYTE_3 src1_sel:DWORD\n\t"
      "v_cndmask_b32_e64 %0, 0, %10, %4\n\t"
      "v_cndmask_b32_e64 %1, 0, %11, %5\n\t"
      "v_cndmask_b32_e64 %2, 0, %12, %6\n\t"
      "v_cndmask_b32_e64 %3, 0, %13, %7"
      : "=&v"(r.x), "=&v"(r.y), "=&v"(r.z), "=&v"(r.w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
      : "v"(id), "v"(j), "v"(d.x), "v"(d.y), "v"(d.z), "v"(d.w));
  return r;
}

// ------------------------------------------------------------------ dgrad A loader (type R)
// Row = conv-INPUT pixel (b, y, x); K = (tap, co).  For one tap the source window, its validity and the
// pixel's position j inside the window are fixed, so with a uniform tap (UT: Co % BK == 0) they are
// recomputed only when the tap changes (every Co/BK K-steps) and a K-step is a scalar add on the two buffer
// bases.  Pixels without a source window (border, stride holes) are BUF_OOB lanes: they read zeros.
template <int NV, int LT, bool UT>
struct ConvDgradA {
  struct Params { const float* dp; const uint8_t* am; int H, W, Hp, Wp, Co, stride, rows, K; };
  struct Raw { float4 d[NV]; uint32_t id[NV]; uint32_t j[NV]; };
  static constexpr bool kTypeR = true;
  Params q;
  int b[NV], y[NV], x[NV];      // x < 0: row past the end
  uint32_t vd[NV], va[NV];      // byte offsets into dp / am of (source window, channel 4*chunk if UT) for the current tap
  uint32_t jc[NV];             // the row's position in its source window for the current tap
  int curtap, c4;
  TapCursor cur;
  __device__ __forceinline__ void init(const Params& q_, int row0, int tid, int ks0) {
    q = q_;
    c4 = 4 * StageMap<LT>::r_chunk(tid);
    cur.init(ks0 * BK + (UT ? 0 : c4), q.Co);
    curtap = -1;
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int m = row0 + StageMap<LT>::r_row(tid, p);
      const int mm = m < q.rows ? m : 0;
      x[p] = m < q.rows ? mm % q.W : -1;
      const int t = mm / q.W;
      y[p] = t % q.H;
      b[p] = t / q.H;
      vd[p] = va[p] = BUF_OOB;
      jc[p] = 0;
    }
  }
  // source window of every row for a tap; c = channel added to the offsets
  __device__ __forceinline__ void retap(int tap, int c) {
    const bool kok = tap < 9;
    const int tp = kok ? tap : 0;
    const int ky = tp / 3, kx = tp - 3 * ky;
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      int yy = y[p] - ky, xx = x[p] - kx;
      bool v = kok && yy >= 0 && xx >= 0;           // x[p] < 0 for rows past the end
      if (q.stride == 2) { v = v && !(yy & 1) && !(xx & 1); yy >>= 1; xx >>= 1; }
      v = v && yy < 2 * q.Hp && xx < 2 * q.Wp;
      const uint32_t e = (uint32_t)((b[p] * q.Hp + (yy >> 1)) * q.Wp + (xx >> 1)) * (uint32_t)q.Co + (uint32_t)c;
      vd[p] = v ? e * 4u : BUF_OOB;
      va[p] = v ? e : BUF_OOB;
      jc[p] = (uint32_t)(((yy & 1) << 1) | (xx & 1));
    }
  }
  __device__ __forceinline__ void issue(int /*ks*/, Raw& r) {
    if (UT) {
      if (cur.tap != curtap) { retap(cur.tap, c4); curtap = cur.tap; }
    } else {
      retap(cur.tap, cur.ch);
    }
    const __amdgpu_buffer_rsrc_t rd = buf_rsrc(q.dp + (UT ? cur.ch : 0)), ra = buf_rsrc(q.am + (UT ? cur.ch : 0));
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      r.d[p] = buf_load16(rd, vd[p]);
      r.id[p] = AM_LOAD(ra, va[p]);
      r.j[p] = jc[p];
    }
    cur.advance();
  }
  __device__ __forceinline__ void finish(const Raw& r, float4 (&o)[NV]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) o[p] = route4(r.d[p], r.id[p], r.j[p]);
  }
};

template <class Cfg, bool U>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void conv_dgrad_kernel(typename ConvDgradA<Cfg::NVA, Cfg::LT, U>::Params pa,
                                                         typename PlainC<Cfg::NVB, Cfg::LT>::Params pb, float* dx,
                                                         int CiP, int tiles_m, int tiles_n, int nk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  const TileCoord tc = tile_coord(tiles_m, tiles_n);
  const int m0 = tc.mt * Cfg::BM, n0 = tc.nt * Cfg::BN;
  using AL = ConvDgradA<Cfg::NVA, Cfg::LT, U>;
  using BL = PlainC<Cfg::NVB, Cfg::LT>;
  f32x16 acc[Cfg::TM][Cfg::TN];
  acc_zero<Cfg>(acc);
  if (!gemm_mainloop<Cfg, AL, BL>(
          [&](AL& al, BL& bl) {
            al.init(pa, m0, loader_tid<Cfg>(), 0);
            bl.init(pb, n0, loader_tid<Cfg>(), 0);
          },
          [](AL&, BL&) {}, acc, 0, nk, pa.K, smem))
    return;
  store_acc_tiles<Cfg>(acc, dx, CiP, pa.rows, CiP, m0, n0, wm, wn, lane);
}

template <class Cfg, bool U>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void conv_dgrad_persistent_kernel(
    typename ConvDgradA<Cfg::NVA, Cfg::LT, U>::Params pa, typename PlainC<Cfg::NVB, Cfg::LT>::Params pb, float* dx, int CiP, int tiles_m,
    int tiles_n, int nk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  using AL = ConvDgradA<Cfg::NVA, Cfg::LT, U>;
  using BL = PlainC<Cfg::NVB, Cfg::LT>;
  gemm_persistent<Cfg, AL, BL, false>(
      xcd_swizzle(blockIdx.x, gridDim.x), gridDim.x, tiles_m * tiles_n, nk, pa.K, smem,
      [&](int t, AL& al, BL& bl) {
        const int mt = t / tiles_n, nt = t - mt * tiles_n;
        al.init(pa, mt * Cfg::BM, loader_tid<Cfg>(), 0);
        bl.init(pb, nt * Cfg::BN, loader_tid<Cfg>(), 0);
      },
      [&](int t, f32x16 (&acc)[Cfg::TM][Cfg::TN]) {
        const int mt = t / tiles_n, nt = t - mt * tiles_n;
        const int m0 = mt * Cfg::BM, n0 = nt * Cfg::BN;
        store_acc_tiles<Cfg>(acc, dx, CiP, pa.rows, CiP, m0, n0, wm, wn, lane);
      });
}

// ------------------------------------------------------------------ wgrad loaders (type C)
struct WgradGeom { int H, W, CiP, Hp, Wp, Co, stride, Mtot; };

// Reduction index m = (b, yo, xo) over the pool-covered conv output [B][2Hp][2Wp]; a lane's pixel
// advances by BK per K-step.  The cursor carries (xo, yo) and a byte offset `off` that its owner keeps in
// step through increments: step_x per K-step, fix_even / fix_odd when the pixel wraps out of an even / odd
// row, fix_img when it wraps into the next image.  A K-step costs a few adds / selects and no multiply.
struct PixelCursor {
  int xo, yo, b, m, Wo2, Ho2;
  bool odd_row;
  uint32_t off, step_x, fix_even, fix_odd, fix_img;
  __device__ __forceinline__ void init(int m_, int Hp, int Wp) {
    Wo2 = 2 * Wp; Ho2 = 2 * Hp; m = m_;
    xo = m_ % Wo2;
    const int t = m_ / Wo2;
    yo = t % Ho2;
    b = t / Ho2;
    odd_row = yo & 1;
    off = step_x = fix_even = fix_odd = fix_img = 0u;
  }
  __device__ __forceinline__ void wrap_row() {
    xo -= Wo2;
    off += odd_row ? fix_odd : fix_even;
    odd_row = !odd_row;
    if (++yo == Ho2) { yo = 0; off += fix_img; }
  }
  __device__ __forceinline__ void advance() {
    m += BK;
    xo += BK;
    off += step_x;
    if (Wo2 >= BK) {                              // uniform: at most one row wrap per K-step, branch-free
      const bool w = xo >= Wo2;
      xo -= w ? Wo2 : 0;
      off += w ? (odd_row ? fix_odd : fix_even) : 0u;
      odd_row = odd_row != w;
      yo += w ? 1 : 0;
      const bool w2 = yo >= Ho2;
      yo -= w2 ? Ho2 : 0;
      off += w2 ? fix_img : 0u;
    } else {
      while (xo >= Wo2) wrap_row();
    }
  }
};

// ---- general wgrad loaders (any channel counts, any image width): per-lane pixel cursor
template <int NV, int LT, bool UF>
struct WgradA {  // A(i = (ky,kx,ci), m) = x[b][yo*s+ky][xo*s+kx][ci]
  struct Params { const float* x; WgradGeom g; int KI; };
  struct Raw { float4 v[NV]; };
  static constexpr bool kTypeR = false;
  Params q;
  uint32_t ioff[NV];       // byte offset of chunk p relative to the pixel (per lane)
  uint32_t su[NV];         // the same for lane 0 of the wave (chunk 0 of its 128-byte line): wave-uniform
  static constexpr bool ufast = false;   // (the uniform case is the specialisation below)
  PixelCursor px;          // px.off = byte offset of the pixel (+ 16 * (lane & 7) when ufast)
  __device__ __forceinline__ void init(const Params& q_, int i0, int tid, int ks0) {
    q = q_;
    px.init(ks0 * BK + StageMap<LT>::c_krow(tid), q.g.Hp, q.g.Wp);
    const uint32_t pix = (uint32_t)(q.g.stride * q.g.CiP) * 4u, row = (uint32_t)q.g.W * pix;
    const uint32_t img = (uint32_t)(q.g.H * q.g.W * q.g.CiP) * 4u;
    px.off = (uint32_t)px.b * img + (uint32_t)px.yo * row + (uint32_t)px.xo * pix + (ufast ? 16u * (uint32_t)(tid & 7) : 0u);
    px.step_x = BK * pix;
    px.fix_even = px.fix_odd = row - (uint32_t)px.Wo2 * pix;    // end of a covered row -> start of the next
    px.fix_img = img - (uint32_t)px.Ho2 * row;                    // below the last covered row -> next image
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int i = i0 + 4 * StageMap<LT>::c_chunk(tid, p);
      const int ii = i < q.KI ? i : 0;     // rows at or beyond KI are never stored: they re-read row 0
      const int tap = ii / q.g.CiP;
      const int ci = ii - tap * q.g.CiP;
      const int ky = tap / 3, kx = tap - 3 * ky;
      ioff[p] = (uint32_t)((ky * q.g.W + kx) * q.g.CiP + ci) * 4u;
      su[p] = __builtin_amdgcn_readfirstlane(ioff[p]);
    }
  }
  __device__ __forceinline__ void issue(int ks, Raw& r) {
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(q.x);
    const bool tail = (ks + 1) * BK > q.g.Mtot;                  // uniform
    if (ufast && !tail) {
#pragma unroll
      for (int p = 0; p < NV; ++p) r.v[p] = buf_load16(rs, px.off, su[p]);
    } else {
      const bool mok = px.m < q.g.Mtot;
#pragma unroll
      for (int p = 0; p < NV; ++p) r.v[p] = buf_load16(rs, mok ? px.off + (ufast ? su[p] : ioff[p]) : BUF_OOB);
    }
    px.advance();
  }
  __device__ __forceinline__ void finish(const Raw& r, float4 (&o)[NV]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) o[p] = r.v[p];
  }
};

template <int NV, int LT, bool UF>
struct WgradB {  // B(m, co) = dY routed from the pooled gradient
  struct Params { const float* dp; const uint8_t* am; WgradGeom g; };
  struct Raw { float4 d[NV]; uint32_t id[NV]; uint32_t j; };
  static constexpr bool kTypeR = false;
  Params q;
  int co[NV];
  uint32_t coff[NV];          // 4 * (co[p] - n0) per lane; BUF_OOB for columns at or beyond Co
  uint32_t j_even;            // j on an even conv-output row (= xo & 1: xo's parity never changes); + 2 on an odd row
  uint32_t bytes;             // of dp from column n0 on
  int n0;
  static constexpr bool ufast = false;   // (the uniform case is the specialisation below)
  PixelCursor px;             // px.off = byte offset in dp of the pixel's window (window row R >> 1, column xo >> 1)
  __device__ __forceinline__ void init(const Params& q_, int n0_, int tid, int ks0) {
    q = q_; n0 = n0_;
    px.init(ks0 * BK + StageMap<LT>::c_krow(tid), q.g.Hp, q.g.Wp);
    const uint32_t win = (uint32_t)q.g.Co * 4u;
    px.off = (uint32_t)(((px.b * px.Ho2 + px.yo) >> 1) * q.g.Wp + (px.xo >> 1)) * win + (ufast ? 16u * (uint32_t)(tid & 7) : 0u);
    px.step_x = (BK / 2) * win;
    px.fix_even = 0u - (uint32_t)q.g.Wp * win;   // even -> odd row: same window row, back to its first window
    px.fix_odd = 0u;                              // odd -> even row: -Wp windows (xo) + Wp windows (next window row)
    px.fix_img = 0u;                              // window rows run on across images
    bytes = (uint32_t)q.g.Mtot * (uint32_t)q.g.Co - 4u * (uint32_t)n0;
    j_even = (uint32_t)(px.xo & 1);
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      co[p] = n0 + 4 * StageMap<LT>::c_chunk(tid, p);
      coff[p] = co[p] < q.g.Co ? 4u * (uint32_t)(co[p] - n0) : BUF_OOB;
    }
  }
  __device__ __forceinline__ void issue(int ks, Raw& r) {
    const bool tail = (ks + 1) * BK > q.g.Mtot;                  // uniform
    r.j = j_even + (px.odd_row ? 2u : 0u);
    // dp / am from column n0 on; a chunk whose columns lie beyond Co reads the next window or, at the very
    // end, past `bytes` (zeros): those columns are never stored
    const __amdgpu_buffer_rsrc_t rd = buf_rsrc(q.dp + n0, bytes), ra = buf_rsrc(q.am + n0, bytes >> 2);
    if (ufast && !tail) {
      const uint32_t pd = px.off, pa = px.off >> 2;
#pragma unroll
      for (int p = 0; p < NV; ++p) {
        r.d[p] = buf_load16(rd, pd + 128u * p);
        r.id[p] = AM_LOAD(ra, pa + 32u * p);
      }
    } else {
      const bool mok = px.m < q.g.Mtot;
#pragma unroll
      for (int p = 0; p < NV; ++p) {
        const uint32_t c = ufast ? 128u * p : coff[p];
        const bool ok = mok && c != BUF_OOB;
        r.d[p] = buf_load16(rd, ok ? px.off + c : BUF_OOB);
        r.id[p] = AM_LOAD(ra, ok ? (px.off + c) >> 2 : BUF_OOB);
      }
    }
    px.advance();
  }
  __device__ __forceinline__ void finish(const Raw& r, float4 (&o)[NV]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      o[p] = route4(r.d[p], r.id[p], r.j);
    }
  }
};

// ---- uniform wgrad loaders: CiP % BK == 0, Co % BK == 0, 2*Wp >= BK, LT == 256
// The K-step's BK consecutive pixels start at a wave-uniform (b, yo, xs) and span at most two rows, so the
// cursor is scalar: a lane's offset is one of two per-lane constants (first / second row) selected by
// kr < n1, added to a scalar base.  The 8 lanes of a 128-byte line share their tap (A: offset in an SGPR)
// and their column group (B: the instruction's immediate).  Per K-step: 2 VALU (A), 4 + routing (B).
struct RowCursor {
  int xs, yo, b, m0, Wo2, Ho2;
  __device__ __forceinline__ void init(int m0_, int Hp, int Wp) {
    Wo2 = 2 * Wp; Ho2 = 2 * Hp; m0 = m0_;
    xs = m0_ % Wo2;
    const int t = m0_ / Wo2;
    yo = t % Ho2;
    b = t / Ho2;
  }
  __device__ __forceinline__ void advance() {
    m0 += BK;
    xs += BK;
    if (xs >= Wo2) { xs -= Wo2; if (++yo == Ho2) { yo = 0; ++b; } }
  }
};

template <int NV, int LT>
struct WgradA<NV, LT, true> {
  struct Params { const float* x; WgradGeom g; int KI; };
  struct Raw { float4 v[NV]; };
  static constexpr bool kTypeR = false;
  Params q;
  uint32_t su[NV];          // byte offset of chunk p's (tap, ci0) relative to the pixel: wave-uniform
  uint32_t lp0, lp1;        // lane constants: kr * pix + 16 * (lane & 7), for the first / second row of a K-step
  uint32_t pix, row, img, fix_img;
  int kr;
  RowCursor rc;
  __device__ __forceinline__ void init(const Params& q_, int i0, int tid, int ks0) {
    q = q_;
    kr = StageMap<LT>::c_krow(tid);
    const int hw = __builtin_amdgcn_readfirstlane(tid >> 8);   // 0 with 4 loader waves; wave-uniform with 8
    rc.init(ks0 * BK, q.g.Hp, q.g.Wp);
    pix = (uint32_t)(q.g.stride * q.g.CiP) * 4u; row = (uint32_t)q.g.W * pix;
    img = (uint32_t)(q.g.H * q.g.W * q.g.CiP) * 4u;
    fix_img = img - (uint32_t)rc.Ho2 * row;
    lp0 = (uint32_t)kr * pix + 16u * (uint32_t)(tid & 7);
    lp1 = lp0 + row - (uint32_t)rc.Wo2 * pix;          // second row: + one row, - the covered width
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int i = i0 + BK * (hw + (LT / 256) * p);      // 128-byte line group of this wave half
      const int ii = i < q.KI ? i : 0;     // rows at or beyond KI are never stored: they re-read row 0
      const int tap = ii / q.g.CiP;
      const int ci = ii - tap * q.g.CiP;
      const int ky = tap / 3, kx = tap - 3 * ky;
      su[p] = (uint32_t)((ky * q.g.W + kx) * q.g.CiP + ci) * 4u;
    }
  }
  __device__ __forceinline__ void issue(int ks, Raw& r) {
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(q.x);
    const int n1 = rc.Wo2 - rc.xs;                                   // pixels left in the first row
    const uint32_t base = (uint32_t)rc.b * img + (uint32_t)rc.yo * row + (uint32_t)rc.xs * pix;
    uint32_t l1 = lp1;
    if (rc.yo + 1 == rc.Ho2 && n1 < BK) l1 += fix_img;             // the second row opens the next image
    const uint32_t off = kr < n1 ? lp0 : l1;
    if ((ks + 1) * BK <= q.g.Mtot) {
#pragma unroll
      for (int p = 0; p < NV; ++p) r.v[p] = buf_load16(rs, off, base + su[p]);
    } else {                                                          // last K-step (or past the end): per-lane validity
      const uint32_t o2 = rc.m0 + kr < q.g.Mtot ? off + base : BUF_OOB;
#pragma unroll
      for (int p = 0; p < NV; ++p) r.v[p] = buf_load16(rs, o2, su[p]);
    }
    rc.advance();
  }
  __device__ __forceinline__ void finish(const Raw& r, float4 (&o)[NV]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) o[p] = r.v[p];
  }
};

template <int NV, int LT>
struct WgradB<NV, LT, true> {
  struct Params { const float* dp; const uint8_t* am; WgradGeom g; };
  struct Raw { float4 d[NV]; uint32_t id[NV]; uint32_t j; };
  static constexpr bool kTypeR = false;
  Params q;
  uint32_t lw0, lwE;        // lane constants: (kr >> 1) * win + 16 * (lane & 7); lwE = lw0 - Wp * win
  uint32_t j0, win;
  int kr, n0, hw;
  RowCursor rc;
  __device__ __forceinline__ void init(const Params& q_, int n0_, int tid, int ks0) {
    q = q_; n0 = n0_;
    kr = StageMap<LT>::c_krow(tid);
    hw = __builtin_amdgcn_readfirstlane(tid >> 8);             // 0 with 4 loader waves; wave-uniform with 8
    rc.init(ks0 * BK, q.g.Hp, q.g.Wp);
    win = (uint32_t)q.g.Co * 4u;
    lw0 = (uint32_t)(kr >> 1) * win + 16u * (uint32_t)(tid & 7);
    lwE = lw0 - (uint32_t)q.g.Wp * win;
    j0 = (uint32_t)(kr & 1);              // xs is always even: the pixel's column parity is the lane's
  }
  __device__ __forceinline__ void issue(int ks, Raw& r) {
    // arg-max tensor = dp bytes / 4 < 0x3fffc000 = BUF_OOB >> 2: its resource ends there
    const __amdgpu_buffer_rsrc_t rd = buf_rsrc(q.dp + n0), ra = buf_rsrc(q.am + n0, BUF_OOB >> 2);
    const int n1 = rc.Wo2 - rc.xs;
    const bool odd = rc.yo & 1;                                      // 2*Hp is even: R = b*2Hp + yo has yo's parity
    const int R = rc.b * rc.Ho2 + rc.yo;
    const uint32_t base = (uint32_t)((R >> 1) * q.g.Wp + (rc.xs >> 1)) * win;
    const bool second = kr >= n1;
    // second row of the K-step: an even row's successor shares its window row (back to its first window),
    // an odd row's successor starts the next window row (which directly follows in memory)
    // lwE alone can be negative (mod 2^32): only the sum with the scalar base is a valid offset
    uint32_t off = (second && !odd ? lwE : lw0) + base;
    r.j = j0 + (second != odd ? 2u : 0u);
    if ((ks + 1) * BK > q.g.Mtot) off = rc.m0 + kr < q.g.Mtot ? off : BUF_OOB;   // last K-step / past the end
    const uint32_t offa = off >> 2;                                  // BUF_OOB >> 2 is past any arg-max tensor (< 1 GiB)
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int grp = hw + (LT / 256) * p;                            // 32-column group of this wave half
      const uint32_t pp = n0 + BK * grp < q.g.Co ? grp : 0;           // uniform; groups past Co are never stored: re-read group 0
      r.d[p] = buf_load16(rd, off, 128u * pp);
      r.id[p] = AM_LOAD(ra, offa, 32u * pp);
    }
    rc.advance();
  }
  __device__ __forceinline__ void finish(const Raw& r, float4 (&o)[NV]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) o[p] = route4(r.d[p], r.id[p], r.j);
  }
};

template <class Cfg, bool U>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void conv_wgrad_kernel(typename WgradA<Cfg::NVA, Cfg::LT, U>::Params pa,
                                                         typename WgradB<Cfg::NVB, Cfg::LT, U>::Params pb, float* slab,
                                                         float* bias_slab, int tiles_m, int tiles_n, int nk,
                                                         int ks_per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  const TileCoord tc = tile_coord(tiles_m, tiles_n);
  const int m0 = tc.mt * Cfg::BM, n0 = tc.nt * Cfg::BN;
  const int split = tc.split;
  const int ks0 = split * ks_per_split;
  const int ks1 = min(nk, ks0 + ks_per_split);
  using AL = WgradA<Cfg::NVA, Cfg::LT, U>;
  using BL = WgradB<Cfg::NVB, Cfg::LT, U>;
  f32x16 acc[Cfg::TM][Cfg::TN];
  acc_zero<Cfg>(acc);
  // bias gradient = column sums of the routed B operand: the MFMA waves of the mt == 0 workgroups add up the B
  // fragments they read anyway (mma_steps CS) -- no accumulators in the loader waves, no second pass over dP
  float cs[Cfg::TN];
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j) cs[j] = 0.f;
  if (!gemm_mainloop<Cfg, AL, BL>(
          [&](AL& al, BL& bl) {
            al.init(pa, m0, loader_tid<Cfg>(), ks0);
            bl.init(pb, n0, loader_tid<Cfg>(), ks0);
          },
          [](AL&, BL&) {}, acc, ks0, ks1, pa.g.Mtot, smem, (tc.mt == 0 && wm == 0) ? cs : nullptr))   // per wave: same barrier count either way
    return;
  if (tc.mt == 0 && wm == 0) {      // one partial bias row per split: lanes of both k halves hold the same column
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const float v = cs[j] + __shfl_xor(cs[j], 32, 64);
      const int col = n0 + acc_col<Cfg>(wn, j, lane);
      if (lane < 32 && col < pa.g.Co) bias_slab[(int64_t)split * pa.g.Co + col] = v;
    }
  }
  const int Co = pa.g.Co;
  float* out = slab + (int64_t)split * pa.KI * Co;
  store_acc_tiles<Cfg>(acc, out, Co, pa.KI, Co, m0, n0, wm, wn, lane);
}

// slab[split][(ky,kx,ciP)][co]  ->  dw[co][ci][ky][kx].  A block covers 64 consecutive slab elements (coalesced
// reads along co); its 4 thread groups take every 4th split and combine through LDS in a fixed order.
static __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* slab, float* dw, int splits, int KI, int CiP,
                                                           int Ci, int Co) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int src = blockIdx.x * 64 + lane;
  const int total = KI * Co;
  float v = 0.f;
  if (src < total)
    for (int s = grp; s < splits; s += 4) v += slab[(int64_t)s * total + src];
  part[grp][lane] = v;
  __syncthreads();
  if (grp == 0 && src < total) {
    v = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    const int co = src % Co;
    const int t = src / Co;
    const int ci = t % CiP;
    const int tap = t / CiP;
    if (ci < Ci) dw[((int64_t)co * Ci + ci) * 9 + tap] = v;
  }
}

// bias_slab[parts][Co] -> dbias[Co]: a block covers 32 columns, its 8 thread groups take every 8th part
static __global__ __launch_bounds__(256) void wgrad_bias_reduce_kernel(const float* bias_slab, float* dbias, int parts, int Co) {
  __shared__ float part[8][32];
  const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + lane;
  float v = 0.f;
  if (c < Co)
    for (int s = grp; s < parts; s += 8) v += bias_slab[(int64_t)s * Co + c];
  part[grp][lane] = v;
  __syncthreads();
  if (grp == 0 && c < Co) {
    v = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) v += part[g][lane];
    dbias[c] = v;
  }
}

static __global__ void pack_weights_kernel(const float* w, float* wf, float* wd, int Co, int Ci, int CiP) {
  const int total = 9 * CiP * Co;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  // e indexes wf: [(tap*CiP + ci)][co]
  const int co = e % Co;
  const int t = e / Co;
  const int ci = t % CiP;
  const int tap = t / CiP;
  const float v = ci < Ci ? w[((int64_t)co * Ci + ci) * 9 + tap] : 0.f;
  wf[e] = v;
  if (wd) wd[((int64_t)tap * Co + co) * CiP + ci] = v;
}

static __global__ void nchw_to_nhwc4_kernel(const float* x, float* y, int C, int64_t HW, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = e / HW, p = e - b * HW;
    const float* s = x + b * C * HW + p;
    float4 v;
    v.x = s[0];
    v.y = C > 1 ? s[HW] : 0.f;
    v.z = C > 2 ? s[2 * HW] : 0.f;
    v.w = C > 3 ? s[3 * HW] : 0.f;
    reinterpret_cast<float4*>(y)[e] = v;
  }
}
