// sk_render.hip — SkillshotGame.get_board (SkillshotGame.py:36-56) for M games
// in one store pass (sk_render_states / sk_env_render, include/skillshot.h).
//
// The output, uint8 [M][W][H], is treated as one flat byte array from its
// 16-byte-aligned base, cut into 16-byte chunks: one lane computes one chunk
// in registers and stores it once (global_store_dwordx4, 1 KiB contiguous per
// wave instruction); the array's last < 16 bytes leave as 8 / 4 / 2 / 1-byte
// stores.  No zero fill followed by sprite stores, no atomics, no ordering
// between lanes: every byte is a function of its board's state.
//
// A workgroup owns a span of consecutive chunks (64 KiB at the reference's
// board size).  Its first lanes read the state of the few boards the span
// touches, once per board, and reduce each to a `Sprites` record in LDS: the
// two players' 5x5 boxes with their pointer cell (the fp64 sincos of the
// rotation is evaluated here, once per board) and the two 3x3 projectile
// boxes, each with the flat [x][y] byte interval that covers its clipped box.
// A chunk is all zero unless it overlaps one of its board's four intervals:
// eight integer compares, wave-uniform but for the wave or two per sprite
// that meet an interval; only those evaluate cells.  A chunk may straddle
// boards (W * H need not be a multiple of 16, or even): those few walk their
// bytes across the board boundary.
//
// Out of range is clipped, not wrapped: a box (partly) off the board
// contributes its on-board cells only, an invalid projectile nothing, a game
// id outside [0, n) an all-zero board (its state is never read).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/skillshot.h"
#include "sk_device.hpp"

namespace {

constexpr int kRenderBlock = 256;
constexpr int kRenderSpan = 4096;  // chunks per workgroup: 16 per lane
constexpr int kRenderCap = 64;     // boards a span may touch (the host shortens the span for small boards)
constexpr int kOffBoard = -16;     // box origin of a sprite with no cell on the board: matches no cell

// one board's sprites in painter's order: 0 = p1 box, 1 = p1 projectile, 2 = p2 box, 3 = p2 projectile
struct Sprites {
  int lo[4], hi[4];  // flat byte interval [lo, hi) of the board covering the clipped box (none: lo = hi = 0)
  int sx[4], sy[4];  // box origin
  int dx[2], dy[2];  // the players' pointer cell inside the 5x5 (-1: not drawn)
};

struct RenderArgs {
  sk::View v;
  int64_t n;           // games behind v
  const int64_t* ids;  // game of board k (NULL: k)
  int64_t m;           // boards
  uint8_t* out;
  int W, H;
  unsigned cells;      // W * H, bytes per board
  int64_t total;       // m * cells
  int64_t chunks;      // ceil(total / 16)
  int span;            // chunks per workgroup
};

__device__ __forceinline__ void set_box(Sprites& d, int s, int x, int y, int size, int W, int H) {
  const int64_t x0 = x > 0 ? x : 0, y0 = y > 0 ? y : 0;
  const int64_t xe = (int64_t)x + size, ye = (int64_t)y + size;
  const int64_t x1 = xe < W ? xe : W, y1 = ye < H ? ye : H;
  if (x0 < x1 && y0 < y1) {
    d.sx[s] = x;
    d.sy[s] = y;
    d.lo[s] = (int)(x0 * H + y0);
    d.hi[s] = (int)((x1 - 1) * H + y1);
  }
}

// the pointer cell (SkillshotGame.py:38-39): floor(-sin(rot) * 5 / 2 + 5 / 2),
// floor(-cos(rot) * 5 / 2 + 5 / 2); index 5 (sin or cos = -1) is no cell
__device__ __forceinline__ void set_pointer(Sprites& d, int p, double rot) {
  bool ok;
  sktrig::SinCos t = sktrig::sincos_bf(rot, &ok);
  if (!ok) t = sk::sincos_lib(rot);  // |rot| >= 1.6e6 or non-finite
  const double fx = floor(((-t.s) * 5.0) / 2.0 + 2.5);
  const double fy = floor(((-t.c) * 5.0) / 2.0 + 2.5);
  if (fx >= 0.0 && fx <= 4.0 && fy >= 0.0 && fy <= 4.0) {  // false for NaN
    d.dx[p] = (int)fx;
    d.dy[p] = (int)fy;
  }
}

__device__ __forceinline__ Sprites board_sprites(const RenderArgs& a, int64_t board) {
  Sprites d;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    d.lo[s] = 0; d.hi[s] = 0;
    d.sx[s] = kOffBoard; d.sy[s] = kOffBoard;
  }
  d.dx[0] = d.dx[1] = d.dy[0] = d.dy[1] = -1;
  const int64_t g = a.ids ? a.ids[board] : board;
  if (g >= 0 && g < a.n) {
    const int4 p = a.v.pos[g];
    const int4 q = a.v.qpos[g];
    const double2 r = a.v.rot[g];
    const unsigned flags = (unsigned)a.v.misc[g].y;
    set_box(d, 0, p.x, p.y, 5, a.W, a.H);
    set_box(d, 2, p.z, p.w, 5, a.W, a.H);
    if (d.hi[0]) set_pointer(d, 0, r.x);
    if (d.hi[2]) set_pointer(d, 1, r.y);
    if (flags & 0xffu) set_box(d, 1, q.x, q.y, 3, a.W, a.H);
    if (flags & 0xff00u) set_box(d, 3, q.z, q.w, 3, a.W, a.H);
  }
  return d;
}

// The painter (SkillshotGame.py:40-55) at one cell, last writer wins.  The
// differences are taken modulo 2^32: a cell is on the board, so a match
// means the true difference is that small.
__device__ __forceinline__ unsigned paint_player(unsigned v, int x, int y, int sx, int sy, int dx, int dy,
                                                 unsigned colour) {
  const unsigned ux = (unsigned)x - (unsigned)sx, uy = (unsigned)y - (unsigned)sy;
  v = ((ux - 1u < 3u) & (uy - 1u < 3u)) ? colour : v;  // Player.py:9-13: the inner 3x3
  v = ((ux < 5u) & (ux == (unsigned)dx) & (uy == (unsigned)dy)) ? colour + 2u : v;
  return v;
}

__device__ __forceinline__ unsigned paint_projectile(unsigned v, int x, int y, int sx, int sy, unsigned colour) {
  const unsigned ux = (unsigned)x - (unsigned)sx, uy = (unsigned)y - (unsigned)sy;
  return ((ux < 3u) & (uy < 3u) & (((ux ^ uy) & 1u) == 0u)) ? colour : v;  // Projectile.py:5-7: the X
}

__device__ __forceinline__ uint4 pack16(const unsigned (&v)[16]) {
  return make_uint4(v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24, v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24,
                    v[8] | v[9] << 8 | v[10] << 16 | v[11] << 24, v[12] | v[13] << 8 | v[14] << 16 | v[15] << 24);
}

// a chunk inside one board that meets the sprites of mask `hit`: bytes p .. p + 15 of the board
__device__ __forceinline__ uint4 render_chunk(const Sprites& d, unsigned hit, unsigned p, int H) {
  int x = (int)(p / (unsigned)H), y = (int)(p - (unsigned)x * (unsigned)H);
  int xs[16], ys[16];
  unsigned v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    xs[i] = x; ys[i] = y; v[i] = 0u;
    if (++y == H) { y = 0; ++x; }
  }
  if (hit & 1u) {
    const int sx = d.sx[0], sy = d.sy[0], dx = d.dx[0], dy = d.dy[0];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = paint_player(v[i], xs[i], ys[i], sx, sy, dx, dy, 1u);
  }
  if (hit & 2u) {
    const int sx = d.sx[1], sy = d.sy[1];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = paint_projectile(v[i], xs[i], ys[i], sx, sy, 3u);
  }
  if (hit & 4u) {
    const int sx = d.sx[2], sy = d.sy[2], dx = d.dx[1], dy = d.dy[1];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = paint_player(v[i], xs[i], ys[i], sx, sy, dx, dy, 2u);
  }
  if (hit & 8u) {
    const int sx = d.sx[3], sy = d.sy[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = paint_projectile(v[i], xs[i], ys[i], sx, sy, 4u);
  }
  return pack16(v);
}

// a chunk that runs past the end of board j (at most one per board, more
// only on boards under 16 cells): `cnt` bytes from byte p of board j, every
// sprite tested at every cell
__device__ __attribute__((noinline)) uint4 render_straddle(const Sprites* D, int j, unsigned p, int cnt, int W,
                                                           int H) {
  int x = (int)(p / (unsigned)H), y = (int)(p - (unsigned)x * (unsigned)H);
  unsigned v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    unsigned c = 0u;
    if (i < cnt) {
      const Sprites& d = D[j];
      c = paint_player(c, x, y, d.sx[0], d.sy[0], d.dx[0], d.dy[0], 1u);
      c = paint_projectile(c, x, y, d.sx[1], d.sy[1], 3u);
      c = paint_player(c, x, y, d.sx[2], d.sy[2], d.dx[1], d.dy[1], 2u);
      c = paint_projectile(c, x, y, d.sx[3], d.sy[3], 4u);
    }
    v[i] = c;
    if (++y == H) {
      y = 0;
      if (++x == W) { x = 0; ++j; }
    }
  }
  return pack16(v);
}

__global__ void __launch_bounds__(kRenderBlock) k_render(const RenderArgs a) {
  __shared__ Sprites D[kRenderCap];
  const unsigned cells = a.cells;
  const int64_t c0 = (int64_t)blockIdx.x * a.span;  // the span: chunks c0 .. c0 + nc - 1, bytes s0 .. s1 - 1
  const int64_t left = a.chunks - c0;
  const int nc = left < a.span ? (int)left : a.span;
  const int64_t s0 = c0 * 16;
  const int64_t s1 = s0 + (int64_t)nc * 16 < a.total ? s0 + (int64_t)nc * 16 : a.total;
  const int64_t b_lo = s0 / cells;  // once per workgroup
  const unsigned r_lo = (unsigned)(s0 - b_lo * cells);
  const int nb = (int)((s1 - 1) / cells - b_lo) + 1;  // <= kRenderCap: the host's choice of span
  if ((int)threadIdx.x < nb) D[threadIdx.x] = board_sprites(a, b_lo + threadIdx.x);
  __syncthreads();

  unsigned p = r_lo + threadIdx.x * 16u;  // the lane's chunk starts at byte p of board b_lo + j
  int j = 0;
  while (p >= cells) { p -= cells; ++j; }
  for (int ci = threadIdx.x; ci < nc; ci += kRenderBlock) {
    const int64_t off = s0 + (int64_t)ci * 16;
    const int64_t rest = a.total - off;
    const int cnt = rest < 16 ? (int)rest : 16;  // 16 but for the array's last chunk
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (p + (unsigned)cnt > cells) {
      w = render_straddle(D, j, p, cnt, a.W, a.H);
    } else {
      const Sprites& d = D[j];
      const unsigned e = p + (unsigned)cnt;
      unsigned hit = 0u;
#pragma unroll
      for (int s = 0; s < 4; ++s) hit |= (unsigned)((p < (unsigned)d.hi[s]) & (e > (unsigned)d.lo[s])) << s;
      if (hit) w = render_chunk(d, hit, p, a.H);
    }
    uint8_t* q = a.out + off;
    if (cnt == 16) {
      *reinterpret_cast<uint4*>(q) = w;
    } else {  // the array's last < 16 bytes
      unsigned long long t = (unsigned long long)w.x | (unsigned long long)w.y << 32;
      if (cnt & 8) {
        *reinterpret_cast<unsigned long long*>(q) = t;
        q += 8;
        t = (unsigned long long)w.z | (unsigned long long)w.w << 32;
      }
      if (cnt & 4) {
        *reinterpret_cast<unsigned*>(q) = (unsigned)t;
        q += 4;
        t >>= 32;
      }
      if (cnt & 2) {
        *reinterpret_cast<unsigned short*>(q) = (unsigned short)t;
        q += 2;
        t >>= 16;
      }
      if (cnt & 1) *q = (uint8_t)t;
    }
    if (ci + kRenderBlock < nc) {
      p += kRenderBlock * 16u;
      while (p >= cells) { p -= cells; ++j; }
    }
  }
}

}  // namespace

// The launch behind sk_render_states (sk_engine.hip validates the arguments:
// planes and out aligned, 0 < W * H < 2^31, m > 0).  hipErrorInvalidValue: more
// workgroups than one launch holds.
hipError_t sk_render_launch(const sk_config& cfg, const sk_state_view& view, const int64_t* ids, int64_t m,
                            uint8_t* out, hipStream_t stream) {
  RenderArgs a;
  a.v.pos = reinterpret_cast<int4*>(view.pos);
  a.v.rot = reinterpret_cast<double2*>(view.rot);
  a.v.qpos = reinterpret_cast<int4*>(view.qpos);
  a.v.qrot = reinterpret_cast<double2*>(view.qrot);
  a.v.qcdage = reinterpret_cast<int4*>(view.qcdage);
  a.v.misc = reinterpret_cast<int2*>(view.misc);
  a.n = view.n_envs;
  a.ids = ids;
  a.m = m;
  a.out = out;
  a.W = cfg.board_w;
  a.H = cfg.board_h;
  const int64_t cells = (int64_t)cfg.board_w * cfg.board_h;
  a.cells = (unsigned)cells;
  a.total = m * cells;
  a.chunks = (a.total + 15) / 16;
  // a span of L bytes touches at most ceil(L / cells) + 1 boards
  const int64_t fit = (kRenderCap - 2) * cells / 16;
  a.span = (int)(fit < kRenderSpan ? fit : kRenderSpan);
  const int64_t grid = (a.chunks + a.span - 1) / a.span;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  k_render<<<dim3((unsigned)grid), dim3(kRenderBlock), 0, stream>>>(a);
  return hipGetLastError();
}
