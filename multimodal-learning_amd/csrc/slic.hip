// SLIC superpixel segmentation of the MIA-2023 masking loader (the reference calls the third-party
// fast_slic once per source tile, "MIA 2023/stage1_multi_modal_teacher/data_loaders_MT_SP.py":303-304:
// Slic(num_components=opt.num_superpixels, compactness=10).iterate(image)).  fast_slic's source is not available: this is a
// segmentation with the same interface and role, NOT bit parity with it.  It is defined in integers only - table-driven
// 8-bit CIELAB, 64-bit integer distances, lowest label on a tie, integer sums - so that the result is exactly
// reproducible and equals the numpy restatement (tests/slic_emulation.py) on every pixel.
//
// Launch sequence of ph_slic (fixed for given shapes, no host synchronisation):
//   table upload (8.5 KB, async) | slic_lab_kernel: uint8 RGB -> one packed Lab word per pixel (written once)
//   | slic_init_kernel: grid centres, sums zeroed | iters x [ slic_assign_kernel | slic_update_kernel (not after the last) ]
// An assignment re-reads the 4-B Lab word and writes a 2-B label per pixel.  A workgroup owns SLIC_CHUNK consecutive
// pixels of one image: the image's centres (2 words each) sit in LDS, every lane handles 4 consecutive pixels (16-B
// load, 8-B store), the per-label sums are packed into two 64-bit LDS accumulators per label (one per wave where the
// whole wave agrees on the label) and leave the workgroup as one 64-bit global atomic per touched label and quantity.
//
// ph_slic_connect, further down: the optional connectivity pass over the label maps (4-connected components by
// union-find, small non-principal components merged into the component above them), seven launches of its own.
#include "ph_common.h"
#include "ph_kernels.h"

namespace {

constexpr int SLIC_MAXN = 2048;       // = SP_MAXN of ph_superpixel_mask, the consumer of the labels
constexpr int SLIC_MAXDIM = 8192;     // H, W: a coordinate fits 13 bits (centre word, packed sums)
constexpr int SLIC_MAXM = 1024;       // compactness
constexpr int SLIC_CHUNK = 4096;      // pixels per workgroup = 256 lanes x 4 pixels x 4 rounds; bounds the packed LDS sums
constexpr int SLIC_NLIN = 256, SLIC_NF = 4096;
constexpr size_t SLIC_TABLE_BYTES = (SLIC_NLIN + SLIC_NF) * sizeof(uint16_t);   // 8704 = 34 x 256

// packed LDS sums of one workgroup (at most SLIC_CHUNK pixels): A = sum L | sum a << 21 | sum b << 42 (each < 2^21),
// Q = count | sum x << 13 | sum y << 38 (count <= 4096 < 2^13, coordinate sums <= 4096 * 8191 < 2^25)
constexpr int SH_A = 21, SH_B = 42, SH_X = 13, SH_Y = 38;
constexpr unsigned long long M21 = (1ull << 21) - 1, M13 = (1ull << 13) - 1, M25 = (1ull << 25) - 1;

// the two host-built tables (float64, once): sRGB byte -> 12-bit linear; 12-bit t -> f(t) of CIELAB in 15-bit fixed point
const uint16_t* slic_host_tables() {
  static uint16_t tab[SLIC_NLIN + SLIC_NF];
  static const bool once = [] {
    for (int v = 0; v < SLIC_NLIN; ++v) {
      const double c = v / 255.0, l = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
      tab[v] = (uint16_t)floor(4095.0 * l + 0.5);
    }
    for (int i = 0; i < SLIC_NF; ++i) {
      const double t = i / 4095.0, f = t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0;
      tab[SLIC_NLIN + i] = (uint16_t)floor(32768.0 * f + 0.5);
    }
    return true;
  }();
  (void)once;
  return tab;
}

// 8-bit Lab (L * 255 / 100, a + 128, b + 128) of one sRGB pixel, packed L | a << 8 | b << 16.  The matrix rows are the
// sRGB -> XYZ rows divided by the D65 white, times 4096, rounded: each row sums to 4096, so grey gives X = Y = Z.
__device__ __forceinline__ uint32_t slic_lab_word(int r, int g, int b, const uint16_t* lin, const uint16_t* ft) {
  const int lr = lin[r], lg = lin[g], lb = lin[b];
  const int fx = ft[(1777 * lr + 1541 * lg + 778 * lb + 2048) >> 12];
  const int fy = ft[(871 * lr + 2929 * lg + 296 * lb + 2048) >> 12];
  const int fz = ft[(73 * lr + 448 * lg + 3575 * lb + 2048) >> 12];
  // L8 = round((116 fy - 16) * 255 / 100) in fixed point 2^15: the numerator is positive (fy >= f(0) = 4520)
  int L = (29580 * fy - 133693440 + 1638400) / 3276800;
  int A = (500 * (fx - fy) + (128 << 15) + (1 << 14)) >> 15;      // arithmetic shift: floor
  int B = (200 * (fy - fz) + (128 << 15) + (1 << 14)) >> 15;
  L = min(max(L, 0), 255); A = min(max(A, 0), 255); B = min(max(B, 0), 255);
  return (uint32_t)L | ((uint32_t)A << 8) | ((uint32_t)B << 16);
}

__global__ __launch_bounds__(256) void slic_lab_kernel(const uint8_t* __restrict__ rgb, uint32_t* __restrict__ lab, size_t npix,
                                                       const uint16_t* __restrict__ tables) {
  __shared__ uint16_t tab[SLIC_NLIN + SLIC_NF];
  for (int i = threadIdx.x; i < (SLIC_NLIN + SLIC_NF) / 2; i += 256)
    reinterpret_cast<uint32_t*>(tab)[i] = reinterpret_cast<const uint32_t*>(tables)[i];
  __syncthreads();
  const uint16_t* lin = tab; const uint16_t* ft = tab + SLIC_NLIN;
  const size_t quads = npix >> 2;                 // 4 pixels = 12 source bytes (three dwords) -> one 16-B store
  const bool wide = (reinterpret_cast<uintptr_t>(rgb) & 3) == 0 && (reinterpret_cast<uintptr_t>(lab) & 15) == 0;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
    if (wide) {
      const uint32_t* s = reinterpret_cast<const uint32_t*>(rgb) + q * 3;
      const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
      u32x4 o;
      o[0] = slic_lab_word(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, lin, ft);
      o[1] = slic_lab_word(w0 >> 24, w1 & 255, (w1 >> 8) & 255, lin, ft);
      o[2] = slic_lab_word((w1 >> 16) & 255, w1 >> 24, w2 & 255, lin, ft);
      o[3] = slic_lab_word((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24, lin, ft);
      *reinterpret_cast<u32x4*>(lab + q * 4) = o;
    } else {
      for (int j = 0; j < 4; ++j) {
        const uint8_t* s = rgb + (q * 4 + j) * 3;
        lab[q * 4 + j] = slic_lab_word(s[0], s[1], s[2], lin, ft);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (npix & 3)) {       // the up to three pixels behind the last quad
    const size_t p = (quads << 2) + threadIdx.x;
    lab[p] = slic_lab_word(rgb[p * 3], rgb[p * 3 + 1], rgb[p * 3 + 2], lin, ft);
  }
}

struct SlicGeo { int H, W, gy, gx, N; };

// centre record: word 0 the packed Lab colour, word 1 = y << 16 | x
__global__ void slic_init_kernel(const uint32_t* __restrict__ lab, u32x2* __restrict__ cen, unsigned long long* __restrict__ sums,
                                 int n, SlicGeo g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * g.N) return;
  const int img = i / g.N, l = i - img * g.N, cy = l / g.gx, cx = l - cy * g.gx;
  const int y = ((2 * cy + 1) * g.H) / (2 * g.gy), x = ((2 * cx + 1) * g.W) / (2 * g.gx);
  u32x2 c;
  c[0] = lab[(size_t)img * g.H * g.W + (size_t)y * g.W + x];
  c[1] = ((uint32_t)y << 16) | (uint32_t)x;
  cen[i] = c;
  for (int k = 0; k < 6; ++k) sums[(size_t)i * 6 + k] = 0;
}

// DT: the integer type of a distance - 32 bits where the host has shown that no distance of the image can reach 2^32
// (the shipped 1024 x 1024 / K = 100 / m = 10 among them), else 64; the values are the same integers either way
template <typename DT> struct SlicBest { DT d; int l; };

// sum of the products of the four bytes of a and b (v_dot4_u32_u8); byte 3 of a Lab word is zero
__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b) { return __builtin_amdgcn_udot4(a, b, 0u, false); }

// distance of a pixel (word w, pp = w . w, dx and dy2 = dy^2 to the centre) to the centre colour c0 (cc = c0 . c0):
// |w - c0|^2 = w . w + c0 . c0 - 2 w . c0, exact in unsigned integers.  Strict <: the first = lowest label of equal distances
template <typename DT>
__device__ __forceinline__ void slic_try(SlicBest<DT>& best, int l, uint32_t c0, uint32_t cc, uint32_t w, uint32_t pp, int dx,
                                         uint32_t dy2, uint32_t S2, uint32_t m2) {
  const uint32_t dc2 = pp + cc - 2u * dot4(w, c0);
  const DT d = (DT)dc2 * S2 + (DT)((uint32_t)(dx * dx) + dy2) * m2;
  if (d < best.d) { best.d = d; best.l = l; }
}

template <typename DT>
__global__ __launch_bounds__(256) void slic_assign_kernel(const uint32_t* __restrict__ lab, const u32x2* __restrict__ cen,
                                                          unsigned long long* __restrict__ sums, int16_t* __restrict__ labels,
                                                          SlicGeo g, uint32_t S2, uint32_t m2, int want_sums) {
  extern __shared__ unsigned long long lds[];          // [2 N] packed sums, then [N] centre records
  unsigned long long* acc = lds;
  u32x2* c = reinterpret_cast<u32x2*>(lds + 2 * g.N);
  const int img = blockIdx.y, tid = threadIdx.x;
  const int HW = g.H * g.W;
  for (int i = tid; i < g.N; i += 256) {
    acc[2 * i] = 0; acc[2 * i + 1] = 0;
    c[i] = cen[(size_t)img * g.N + i];
  }
  __syncthreads();
  const uint32_t* src = lab + (size_t)img * HW;
  int16_t* dst = labels + (size_t)img * HW;
  const bool wide = (HW & 3) == 0;                      // then every quad of every image is 16-B / 8-B aligned
  for (int round = 0; round < SLIC_CHUNK / 1024; ++round) {
    const int p = blockIdx.x * SLIC_CHUNK + (round * 256 + tid) * 4;
    const int cnt = min(4, HW - p);                     // <= 0: this lane is behind the image
    uint32_t w[4] = {0, 0, 0, 0};
    int lb[4] = {-1, -1, -1, -1}, ys[4] = {0, 0, 0, 0}, xs[4] = {0, 0, 0, 0}, hys[4], hxs[4];
    if (cnt > 0) {
      if (wide) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(src + p);
        w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) w[j] = src[p + j];
      }
      int y = p / g.W, x = p - y * g.W, hy = (y * g.gy) / g.H, hx = (x * g.gx) / g.W;
#pragma unroll
      for (int j = 0; j < 4; ++j) {                     // home cells ((y gy) / H, (x gx) / W), stepped without divisions
        ys[j] = y; xs[j] = x; hys[j] = hy; hxs[j] = hx;
        if (++x == g.W) {
          x = 0; hx = 0; ++y;
          if (y * g.gy >= (hy + 1) * g.H) ++hy;
        } else if (x * g.gx >= (hx + 1) * g.W) ++hx;
      }
      SlicBest<DT> best[4];
      uint32_t pp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { best[j].d = ~(DT)0; best[j].l = 0; pp[j] = dot4(w[j], w[j]); }
      if (cnt == 4 && ys[0] == ys[3] && hxs[0] == hxs[3]) {
        // the four pixels lie in one row and share their home cell (the common case; hx does not decrease along a
        // row): each of the up to nine centres is read and unpacked once, the row term is shared
        for (int cy = max(hys[0] - 1, 0); cy <= min(hys[0] + 1, g.gy - 1); ++cy)
          for (int cx = max(hxs[0] - 1, 0); cx <= min(hxs[0] + 1, g.gx - 1); ++cx) {
            const int l = cy * g.gx + cx;
            const u32x2 k = c[l];
            const uint32_t cc = dot4(k[0], k[0]);
            const int dy = ys[0] - (int)(k[1] >> 16), x0 = xs[0] - (int)(k[1] & 0xffff);
            const uint32_t dy2 = (uint32_t)(dy * dy);
#pragma unroll
            for (int j = 0; j < 4; ++j) slic_try(best[j], l, k[0], cc, w[j], pp[j], x0 + j, dy2, S2, m2);
          }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= cnt) continue;
          for (int cy = max(hys[j] - 1, 0); cy <= min(hys[j] + 1, g.gy - 1); ++cy)
            for (int cx = max(hxs[j] - 1, 0); cx <= min(hxs[j] + 1, g.gx - 1); ++cx) {
              const int l = cy * g.gx + cx;
              const u32x2 k = c[l];
              const int dy = ys[j] - (int)(k[1] >> 16);
              slic_try(best[j], l, k[0], dot4(k[0], k[0]), w[j], pp[j], xs[j] - (int)(k[1] & 0xffff), (uint32_t)(dy * dy), S2, m2);
            }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) lb[j] = j < cnt ? best[j].l : -1;
      if (wide) {
        s16x4 o;
        o[0] = (short)lb[0]; o[1] = (short)lb[1]; o[2] = (short)lb[2]; o[3] = (short)lb[3];
        *reinterpret_cast<s16x4*>(dst + p) = o;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) dst[p + j] = (int16_t)lb[j];
      }
    }
    if (!want_sums) continue;
    // sums: merge the lane's run of equal labels, then one LDS atomic pair per wave where all 256 pixels of the wave
    // carry one label, else one pair per lane and run
    unsigned long long A[4], Q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      A[j] = (unsigned long long)(w[j] & 255) | ((unsigned long long)((w[j] >> 8) & 255) << SH_A) |
             ((unsigned long long)((w[j] >> 16) & 255) << SH_B);
      Q[j] = lb[j] < 0 ? 0ull : (1ull | ((unsigned long long)xs[j] << SH_X) | ((unsigned long long)ys[j] << SH_Y));
      if (lb[j] < 0) A[j] = 0;
    }
    const bool lane_one = lb[0] >= 0 && lb[0] == lb[1] && lb[0] == lb[2] && lb[0] == lb[3];
    const int first = __builtin_amdgcn_readfirstlane(lb[0]);
    if (__all(lane_one && lb[0] == first)) {
      const unsigned long long a = wave_sum_u64(A[0] + A[1] + A[2] + A[3]), q = wave_sum_u64(Q[0] + Q[1] + Q[2] + Q[3]);
      if ((tid & 63) == 0) { atomicAdd(&acc[2 * first], a); atomicAdd(&acc[2 * first + 1], q); }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (lb[j] < 0) continue;
        if (j < 3 && lb[j + 1] == lb[j]) { A[j + 1] += A[j]; Q[j + 1] += Q[j]; continue; }
        atomicAdd(&acc[2 * lb[j]], A[j]); atomicAdd(&acc[2 * lb[j] + 1], Q[j]);
      }
    }
  }
  if (!want_sums) return;
  __syncthreads();
  for (int l = tid; l < g.N; l += 256) {
    const unsigned long long q = acc[2 * l + 1];
    if (!q) continue;                                   // count 0: label not touched by this workgroup
    const unsigned long long a = acc[2 * l];
    unsigned long long* s = sums + ((size_t)img * g.N + l) * 6;
    atomicAdd(s + 0, a & M21); atomicAdd(s + 1, (a >> SH_A) & M21); atomicAdd(s + 2, a >> SH_B);
    atomicAdd(s + 3, q >> SH_Y); atomicAdd(s + 4, (q >> SH_X) & M25); atomicAdd(s + 5, q & M13);
  }
}

// centre := rounded integer mean (2 sum + n) / (2 n) of L, a, b, y, x; a label without pixels keeps its centre; sums zeroed
__global__ void slic_update_kernel(u32x2* __restrict__ cen, unsigned long long* __restrict__ sums, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  unsigned long long* s = sums + (size_t)i * 6;
  const unsigned long long n = s[5];
  if (n) {
    uint32_t m[5];
    for (int k = 0; k < 5; ++k) m[k] = (uint32_t)((2 * s[k] + n) / (2 * n));
    u32x2 c;
    c[0] = m[0] | (m[1] << 8) | (m[2] << 16);
    c[1] = (m[3] << 16) | m[4];
    cen[i] = c;
  }
  for (int k = 0; k < 6; ++k) s[k] = 0;
}

// gy = floor(sqrt(K H / W)) as the largest g with g g W <= K H; gx = K / gy
bool slic_geo(int H, int W, int K, SlicGeo& g) {
  if (H < 1 || W < 1 || K < 1 || H > SLIC_MAXDIM || W > SLIC_MAXDIM) return false;
  long long gy = 1;
  while ((gy + 1) * (gy + 1) * (long long)W <= (long long)K * H) ++gy;
  const long long gx = K / gy;
  if (gx < 1 || gy > H || gx > W || gy * gx > SLIC_MAXN) return false;
  g.H = H; g.W = W; g.gy = (int)gy; g.gx = (int)gx; g.N = (int)(gy * gx);
  return true;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// ------------------------------------------------------------------------------------------------------------------
// Connectivity pass (ph_slic_connect): 4-connected components of equal labels by union-find whose
// root is the LOWEST raster index of the component (its first pixel), then every small non-principal component takes
// the final label of the component above (in row 0: left of) its first pixel.  Integers only; every sum, minimum and
// maximum is an integer atomic, so the result does not depend on the order in which they land.
//
// Per tile two words per pixel, P (parent, later root: a tile-local raster index) and S (size at a root, later its
// link: the root whose label it takes), and one 64-bit word per label (the principal component's key).  Launches:
//   cc_local_kernel   a CC_BW x CC_BH block of the tile resolved in LDS -> P = block-local root, S = its pixel count there
//   cc_seam_kernel    equal labels across the right and lower block seams united: atomicMin on P
//   cc_flatten_kernel P := root; block-local counts added into S[root]
//   cc_principal_kernel  per (tile, label) the maximum of size << 32 | ~first over the roots
//   cc_target_kernel  S[root] := root of the pixel above / left of it where the component is merged, else itself
//   cc_chain_kernel   S[root] := end of its chain of links
//   cc_relabel_kernel out[p] = in[S[P[p]]]
// Every loop either walks to a strictly lower index (parents and links point downwards) or has a fixed count; no
// workgroup waits for another.  Phases that read what other workgroups wrote are separated by kernel boundaries; where
// a word is read while other workgroups update it (the seam union, the chain compression) every access to it is an
// agent-scope atomic.
constexpr int CC_BW = 64, CC_BH = 16, CC_PIX = CC_BW * CC_BH;      // 256 lanes x 4 consecutive pixels of one row
constexpr int CC_FLAT = 1024;                                       // pixels per workgroup of the flat kernels

struct CcGeo { int H, W, N, bxn; };

__device__ __forceinline__ uint32_t cc_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x: parents are <= their child, so the walk is strictly downwards and ends at the latest at index 0
__device__ __forceinline__ uint32_t cc_find(const uint32_t* P, uint32_t x) {
  for (;;) {
    const uint32_t q = cc_ld(P + x);
    if (q >= x) return x;
    x = q;
  }
}

// unite the trees of a and b under the lower root.  Each round either ends or replaces the higher root by a strictly
// lower index (the parent another workgroup has given it meanwhile)
__device__ __forceinline__ void cc_union(uint32_t* P, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find(P, a); b = cc_find(P, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(P + a, b);
    if (old >= a) return;                                 // a was a root: now linked (old > a cannot happen)
    a = old;
  }
}

__device__ __forceinline__ uint32_t lds_find(const uint32_t* lp, uint32_t x) {
  for (;;) {
    const uint32_t q = __hip_atomic_load(lp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (q >= x) return x;
    x = q;
  }
}

__device__ __forceinline__ void lds_union(uint32_t* lp, uint32_t a, uint32_t b) {
  for (;;) {
    a = lds_find(lp, a); b = lds_find(lp, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(lp + a, b);
    if (old >= a) return;
    a = old;
  }
}

constexpr int CC_OUTSIDE = 1 << 20;      // label of a block position outside the image: equal to no int16 label

__global__ __launch_bounds__(256) void cc_local_kernel(const int16_t* __restrict__ labels, uint32_t* __restrict__ P,
                                                       uint32_t* __restrict__ S, unsigned long long* __restrict__ best, CcGeo g) {
  __shared__ int lab[CC_PIX];
  __shared__ uint32_t lp[CC_PIX], cnt[CC_PIX];
  const int tid = threadIdx.x, tile = blockIdx.y;
  const int by = blockIdx.x / g.bxn, bx = blockIdx.x - by * g.bxn;
  const size_t base = (size_t)tile * g.H * g.W;
  if (blockIdx.x == 0)
    for (int l = tid; l < g.N; l += 256) best[(size_t)tile * g.N + l] = 0;
  const int ly = tid >> 4, lx0 = (tid & 15) * 4, y = by * CC_BH + ly, x0 = bx * CC_BW + lx0, i0 = ly * CC_BW + lx0;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = (y < g.H && x0 + j < g.W) ? (int)labels[base + (size_t)y * g.W + x0 + j] : CC_OUTSIDE + i0 + j;
    lab[i0 + j] = v[j];
    cnt[i0 + j] = 0;
  }
  // the lane's run of equal labels starts linked to its first pixel
  uint32_t par[4];
  par[0] = i0;
#pragma unroll
  for (int j = 1; j < 4; ++j) par[j] = v[j] == v[j - 1] ? par[j - 1] : i0 + j;
#pragma unroll
  for (int j = 0; j < 4; ++j) lp[i0 + j] = par[j];
  __syncthreads();
  if (lx0 + 4 < CC_BW && lab[i0 + 4] == v[3]) lds_union(lp, i0 + 3, i0 + 4);
  if (ly + 1 < CC_BH) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lab[i0 + j + CC_BW] == v[j] && (j == 0 || v[j] != v[j - 1] || lab[i0 + j - 1 + CC_BW] != v[j]))
        lds_union(lp, i0 + j, i0 + j + CC_BW);           // (skipped where the pair to the left already joins the two runs)
  }
  __syncthreads();
  uint32_t r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = lds_find(lp, i0 + j);
  __syncthreads();
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lp[i0 + j] = r[j];
    ++run;
    if (j == 3 || r[j + 1] != r[j]) { atomicAdd(&cnt[r[j]], run); run = 0; }
  }
  __syncthreads();
  if (y >= g.H) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (x0 + j >= g.W) break;
    const uint32_t rt = r[j], ry = rt / CC_BW, rx = rt - ry * CC_BW;
    const size_t p = base + (size_t)y * g.W + x0 + j;
    P[p] = (uint32_t)((by * CC_BH + (int)ry) * g.W + bx * CC_BW + (int)rx);
    S[p] = rt == (uint32_t)(i0 + j) ? cnt[rt] : 0u;
  }
}

// lanes 0 .. CC_BW - 1: the pairs across the lower seam of the block, lanes CC_BW .. CC_BW + CC_BH - 1: across its right seam
__global__ __launch_bounds__(128) void cc_seam_kernel(const int16_t* __restrict__ labels, uint32_t* __restrict__ P, CcGeo g) {
  const int tid = threadIdx.x, tile = blockIdx.y;
  const int by = blockIdx.x / g.bxn, bx = blockIdx.x - by * g.bxn;
  int y, x, y2, x2;
  if (tid < CC_BW) { y = by * CC_BH + CC_BH - 1; x = bx * CC_BW + tid; y2 = y + 1; x2 = x; }
  else if (tid < CC_BW + CC_BH) { y = by * CC_BH + tid - CC_BW; x = bx * CC_BW + CC_BW - 1; y2 = y; x2 = x + 1; }
  else return;
  if (y2 >= g.H || x2 >= g.W) return;
  const size_t base = (size_t)tile * g.H * g.W;
  const uint32_t a = (uint32_t)(y * g.W + x), b = (uint32_t)(y2 * g.W + x2);
  if (labels[base + a] != labels[base + b]) return;
  cc_union(P + base, a, b);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(uint32_t* __restrict__ P, uint32_t* __restrict__ S, CcGeo g) {
  const int HW = g.H * g.W;
  const int p0 = blockIdx.x * CC_FLAT + threadIdx.x;     // pixel j of a lane: p0 + 256 j (coalesced)
  uint32_t* Pt = P + (size_t)blockIdx.y * HW;
  uint32_t* St = S + (size_t)blockIdx.y * HW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + 256 * j;
    if (p >= HW) return;
    const uint32_t r = cc_find(Pt, (uint32_t)p);
    if (r == (uint32_t)p) continue;
    Pt[p] = r;                                           // any parent another lane still reads here is an ancestor either way
    const uint32_t c = St[p];                            // block-local count: only roots' words are added to
    if (c) atomicAdd(St + r, c);
  }
}

__device__ __forceinline__ unsigned long long cc_key(uint32_t size, uint32_t first) {
  return ((unsigned long long)size << 32) | (0xFFFFFFFFu - first);
}

__global__ __launch_bounds__(256) void cc_principal_kernel(const int16_t* __restrict__ labels, const uint32_t* __restrict__ P,
                                                           const uint32_t* __restrict__ S, unsigned long long* __restrict__ best, CcGeo g) {
  const int HW = g.H * g.W;
  const int p0 = blockIdx.x * CC_FLAT + threadIdx.x;     // pixel j of a lane: p0 + 256 j (coalesced)
  const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + 256 * j;
    if (p >= HW) return;
    if (P[base + p] != (uint32_t)p) continue;
    const int l = labels[base + p];
    if (l < 0 || l >= g.N) continue;                     // a label outside the table: never merged, never principal
    // (reading the word first to skip keys that cannot win was measured: the agent-scope loads of the hot words cost
    // more than the atomics they save, 1.51 ms against 0.58 ms per 64 tiles of 1024 x 1024)
    atomicMax(best + (size_t)blockIdx.y * g.N + l, cc_key(S[base + p], (uint32_t)p));
  }
}

__global__ __launch_bounds__(256) void cc_target_kernel(const int16_t* __restrict__ labels, const uint32_t* __restrict__ P,
                                                        uint32_t* __restrict__ S, const unsigned long long* __restrict__ best, CcGeo g,
                                                        uint32_t min_size) {
  const int HW = g.H * g.W;
  const int p0 = blockIdx.x * CC_FLAT + threadIdx.x;     // pixel j of a lane: p0 + 256 j (coalesced)
  const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + 256 * j;
    if (p >= HW) return;
    if (P[base + p] != (uint32_t)p) continue;
    const int l = labels[base + p];
    const uint32_t size = S[base + p];
    uint32_t link = (uint32_t)p;
    if (p > 0 && size < min_size && l >= 0 && l < g.N && best[(size_t)blockIdx.y * g.N + l] != cc_key(size, (uint32_t)p))
      link = P[base + (p >= g.W ? p - g.W : p - 1)];     // the root of the component above (row 0: left of) the first pixel
    S[base + p] = link;
  }
}

// links point to strictly lower roots and end at a root linked to itself; the ends never change, so compressing in
// place is safe whatever another lane has already compressed
__global__ __launch_bounds__(256) void cc_chain_kernel(const uint32_t* __restrict__ P, uint32_t* __restrict__ S, CcGeo g) {
  const int HW = g.H * g.W;
  const int p0 = blockIdx.x * CC_FLAT + threadIdx.x;     // pixel j of a lane: p0 + 256 j (coalesced)
  const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + 256 * j;
    if (p >= HW) return;
    if (P[base + p] != (uint32_t)p) continue;
    uint32_t f = cc_ld(S + base + p);
    if (f >= (uint32_t)p) continue;
    const uint32_t first = f;
    for (;;) {
      const uint32_t q = cc_ld(S + base + f);
      if (q >= f) break;
      f = q;
    }
    if (f != first) __hip_atomic_store(S + base + p, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the pixel of a chain's end belongs to a component that keeps its label, so reading it while labels_out == labels_in
// is written reads the same value before and after
__global__ __launch_bounds__(256) void cc_relabel_kernel(const int16_t* labels_in, int16_t* labels_out, const uint32_t* __restrict__ P,
                                                         const uint32_t* __restrict__ S, CcGeo g) {
  const int HW = g.H * g.W;
  const int p0 = blockIdx.x * CC_FLAT + threadIdx.x;     // pixel j of a lane: p0 + 256 j (coalesced)
  const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + 256 * j;
    if (p >= HW) return;
    const uint32_t r = P[base + p];
    const uint32_t f = r < (uint32_t)HW ? S[base + r] : (uint32_t)p;
    labels_out[base + p] = labels_in[base + (f < (uint32_t)HW ? f : (uint32_t)p)];
  }
}

bool cc_args(int n, int H, int W, int N) {
  return n >= 1 && n <= 65535 && H >= 1 && W >= 1 && H <= SLIC_MAXDIM && W <= SLIC_MAXDIM && N >= 1 && N <= SLIC_MAXN;
}

}  // namespace

#include "pathomic_hip.h"

extern "C" {

int ph_slic_num_labels(int H, int W, int K) {
  SlicGeo g;
  return slic_geo(H, W, K, g) ? g.N : PH_EINVAL;
}

size_t ph_slic_workspace_bytes(int n, int H, int W, int K) {
  SlicGeo g;
  if (n < 1 || !slic_geo(H, W, K, g)) return 0;
  return SLIC_TABLE_BYTES + up256((size_t)n * H * W * sizeof(uint32_t)) + up256((size_t)n * g.N * sizeof(u32x2)) +
         up256((size_t)n * g.N * 6 * sizeof(unsigned long long));
}

int ph_slic_lab(const uint8_t* rgb, uint32_t* lab, size_t npix, void* workspace, hipStream_t st) {
  if (!rgb || !lab || !workspace || npix < 1) return PH_EINVAL;
  if (hipMemcpyAsync(workspace, slic_host_tables(), SLIC_TABLE_BYTES, hipMemcpyHostToDevice, st) != hipSuccess) return PH_ELAUNCH;
  const size_t blocks = ((npix >> 2) + 255) / 256;
  hipLaunchKernelGGL(slic_lab_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks))), dim3(256), 0, st, rgb, lab,
                     npix, (const uint16_t*)workspace);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_slic(const uint8_t* tiles, int16_t* labels, int n, int H, int W, int K, int compactness, int iters, void* workspace,
            hipStream_t st) {
  SlicGeo g;
  if (!tiles || !labels || !workspace || n < 1 || n > 65535 || iters < 1 || compactness < 0 || compactness > SLIC_MAXM ||
      !slic_geo(H, W, K, g))
    return PH_EINVAL;
  const size_t npix = (size_t)n * H * W;
  char* ws = (char*)workspace;
  uint32_t* lab = (uint32_t*)(ws + SLIC_TABLE_BYTES);
  u32x2* cen = (u32x2*)((char*)lab + up256(npix * sizeof(uint32_t)));
  unsigned long long* sums = (unsigned long long*)((char*)cen + up256((size_t)n * g.N * sizeof(u32x2)));
  int rc = ph_slic_lab(tiles, lab, npix, workspace, st);
  if (rc != PH_OK) return rc;
  const int total = n * g.N;
  hipLaunchKernelGGL(slic_init_kernel, dim3((total + 255) / 256), dim3(256), 0, st, lab, cen, sums, n, g);
  PH_LAUNCH_CHECK();
  const uint32_t S2 = (uint32_t)(((long long)H * W) / g.N), m2 = (uint32_t)(compactness * compactness);
  // the largest distance any pixel of the image can have: 3 * 255^2 in colour, the image diagonal in space
  const bool narrow = 195075ull * S2 + (unsigned long long)m2 * ((unsigned long long)H * H + (unsigned long long)W * W) < (1ull << 32);
  const dim3 grid((H * W + SLIC_CHUNK - 1) / SLIC_CHUNK, n);
  const size_t lds = (size_t)g.N * (2 * sizeof(unsigned long long) + sizeof(u32x2));   // <= 48 KiB
  for (int it = 0; it < iters; ++it) {
    const int last = it == iters - 1;
    if (narrow) hipLaunchKernelGGL(slic_assign_kernel<uint32_t>, grid, dim3(256), lds, st, lab, cen, sums, labels, g, S2, m2, !last);
    else hipLaunchKernelGGL(slic_assign_kernel<unsigned long long>, grid, dim3(256), lds, st, lab, cen, sums, labels, g, S2, m2, !last);
    PH_LAUNCH_CHECK();
    if (last) break;
    hipLaunchKernelGGL(slic_update_kernel, dim3((total + 255) / 256), dim3(256), 0, st, cen, sums, total);
    PH_LAUNCH_CHECK();
  }
  return PH_OK;
}

size_t ph_slic_connect_workspace_bytes(int n, int H, int W, int N) {
  if (!cc_args(n, H, W, N)) return 0;
  return 2 * up256((size_t)n * H * W * sizeof(uint32_t)) + up256((size_t)n * N * sizeof(unsigned long long));
}

int ph_slic_connect(const int16_t* labels_in, int16_t* labels_out, int n, int H, int W, int N, int min_size, void* workspace,
                    hipStream_t st) {
  if (!labels_in || !labels_out || !workspace || min_size < 1 || !cc_args(n, H, W, N)) return PH_EINVAL;
  const size_t words = up256((size_t)n * H * W * sizeof(uint32_t));
  uint32_t* P = (uint32_t*)workspace;
  uint32_t* S = (uint32_t*)((char*)workspace + words);
  unsigned long long* best = (unsigned long long*)((char*)workspace + 2 * words);
  CcGeo g;
  g.H = H; g.W = W; g.N = N; g.bxn = (W + CC_BW - 1) / CC_BW;
  const dim3 blocks(g.bxn * ((H + CC_BH - 1) / CC_BH), n), flat((H * W + CC_FLAT - 1) / CC_FLAT, n);
  hipLaunchKernelGGL(cc_local_kernel, blocks, dim3(256), 0, st, labels_in, P, S, best, g);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_seam_kernel, blocks, dim3(128), 0, st, labels_in, P, g);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, flat, dim3(256), 0, st, P, S, g);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_principal_kernel, flat, dim3(256), 0, st, labels_in, (const uint32_t*)P, (const uint32_t*)S, best, g);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_target_kernel, flat, dim3(256), 0, st, labels_in, (const uint32_t*)P, S, (const unsigned long long*)best, g,
                     (uint32_t)min_size);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_chain_kernel, flat, dim3(256), 0, st, (const uint32_t*)P, S, g);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_relabel_kernel, flat, dim3(256), 0, st, labels_in, labels_out, (const uint32_t*)P, (const uint32_t*)S, g);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

}  // extern "C"
