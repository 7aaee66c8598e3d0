// sweep_rect.hip -- the fixed sampler's plane sweep (arithmetic contract v2, sweep_fx.hip / DESIGN.md section 2b) for RECTIFIED side
// views on gfx950: the same cells, bit for bit, at a third of the vector instructions.
//
// A side view is "rectified" against the main view when its matrix Q (csrc/camera_math.cpp) has q1 = q4 = q8 = q9 = q10 = 0: the
// side camera is a pure translation of the main one inside its focal plane with the same intrinsics -- the classic fronto-parallel
// plane sweep, and SURVEY.md section 8d's benchmark ring.  Then, in the contract's own f32 arithmetic,
//     Tx = fma(fma(z, bx, fma(q0, xn, q3)), 256 r, magic + 4)      depends on (column, plane, view) only
//     Ty = fma(fma(z, by, fma(q5, yn, q7)), 256 r, magic + 4)      depends on (row, plane, view) only,  r = RN(1 / q11) per view
// and in exact arithmetic both advance by exactly 256 per pixel: every pixel of a plane samples the side view at the SAME sub-texel
// phase (kx, ky) and at the texel its own position plus one common shift.  The f32 roundings break that on a few per cent of the
// (plane, view) pairs (a coordinate within ~0.07 / 256 texel of a rounding boundary).  So a planner kernel EVALUATES the contract's
// expression for every column of a 64-column tile (and every row of an 8-row tile) and records, per (tile column, view, plane) and
// per (tile row, view, plane), the first pixel's integer texel and phase plus two certificates: "every pixel of the tile is in frame"
// and "every pixel has the view's nominal phase and the texel of the first pixel plus its own offset".  Where both hold -- 96-98 % of
// the (wavefront, plane, view) triples -- the sweep kernel needs NO per-lane coordinate arithmetic at all:
//     quad   = LDS[slot + (iy - y0 + j) * RS + (ix - x0) + lane]          one ds_read_b32 at a wave-uniform base + lane
//     cell  += |v_dot4_u32_u8(quad, W[ky][kx]) - 255 I_main|               weight word in an SGPR; v_dot4 + v_sad_u16 = 2 VALU / sample
// (sweep_fx_tiled: 9.25 in its sample loop, 12.4 overall).  Where a certificate fails, that plane of that wavefront evaluates the
// general expression per lane with texels gathered from the view's quad image in global memory (`slow_plane`): the same function of
// the same inputs, so the two kernels agree on every cell (tests/test_sweep_gpu.py: rect vs general vs oracle).
//
// Thread mapping.  Workgroup = 256 threads = one 64 x 8-pixel tile x one 16-plane chunk, as in sweep_fx_tiled (same planner boxes);
// but a wavefront owns ALL 8 rows of the tile and 4 of the 16 planes (lane = column): 32 accumulators per thread, and a plane's
// uniform work (decode, weight word, LDS base) is shared by 8 rows.
//
// Region pipeline.  Per (chunk, view) the planner's box of the view's quad image is copied into one of two LDS slots by
// buffer_load_dwordx4 ... lds (dense rows of RS quads, 1 KiB = 64 lanes x 16 B per instruction, per-lane source offsets fixed for the
// launch), one region ahead of the one being sampled; s_waitcnt vmcnt(0) + one s_barrier per region make every wavefront's part
// visible and free the slot the next copy goes to.  The copies carry no lane mask: they go through a buffer resource that ends with
// the box's last row, and the range check drops the lanes past it.  The X / Y records lie in the order a workgroup takes its regions
// (the next region's records are the next 256 bytes), travel through vector registers one region ahead (lane l = dword l), are added
// lane by lane when the region's turn comes, and every scalar of the turn -- the four LDS offsets, the four weight words, the clean
// test, the source and the end of the NEXT region's copy -- is one v_readlane of the sum with no arithmetic behind it
// (plan_rect_pack).  A region's sampling is inline asm in two shapes, chosen by one wave-uniform test
// per region: CLEAN (all four planes FULL) is one straight-line statement for the four planes, the next plane's reads in flight behind
// the current plane's arithmetic; otherwise one statement per plane (M0-based ds_read_addtid_b32, v_dot4_u32_u8, v_sad_u16; border
// planes under EXEC masks, planes with nothing in frame branched over) plus the block for failed certificates.  Not compiler code: the
// compiler would order every ds_read behind ALL pending LDS copies.
// The chunk epilogue (the 32 cost volume stores of a wavefront and its depth selection over its four planes) does not run where the
// chunk's last view has been sampled -- the next instruction there is the full wait, and stores count in vmcnt like the copies -- but
// one turn later, behind the barrier and the issue of the next copy and in front of the sampling: the write acknowledgements then
// have a region's sampling to come back in.  The workgroup's last chunk is finished behind the loop.
// What bounds it (profiles/r03): vector-instruction issue.  Measured and rejected: a second region of look-ahead
// with counted waits (three slots, records through an LDS ring; +10 %), row-wise copies (+8 %), copies that all hit in L2 (no change).
#include "sweep_shared.hpp"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <type_traits>
#include <vector>

namespace mvs {

namespace {

constexpr float RX_MAGIC = 12582912.0f;  // 1.5 * 2^23 (FX_MAGIC of sweep_fx.hip)
constexpr int RX_TILE_H = 8, RX_PC = 16, RX_KW = 4;  // tile rows, planes per chunk, planes per wavefront
constexpr int RX_MAX_NI = 3;                          // copy instructions per wavefront and region, at most
#ifndef RX_DOUBLE_BUFFER
#define RX_DOUBLE_BUFFER 0
#endif
#ifndef RX_WAVES
#define RX_WAVES 5
#endif
constexpr int RX_WAVES_PER_SIMD = RX_WAVES;                  // launch bound: <= 128 VGPRs

enum RxMode : unsigned { RX_SKIP = 0, RX_FAST = 1, RX_BORDER = 2, RX_GENERIC = 3 };  // = FxMode (the plan is plan_regions_fx's)

constexpr uint32_t RX_UNIFORM = 1u << 30;

// Read-only tables are read through the CONSTANT address space: a wave-uniform load from it is a scalar load (s_load_dword*)
// whatever the kernel stores elsewhere (through a global pointer the compiler must assume the volume stores may alias it and
// falls back to vector loads after the first store).
typedef const __attribute__((address_space(4))) uint32_t *cu32;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x2 *cu2;
typedef const __attribute__((address_space(4))) u32x4 *cu4;
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(4))) u32x8 *cu8;
typedef const __attribute__((address_space(4))) float *cf32;
template <typename T, typename U>
__device__ __forceinline__ T as_const(const U *p) { return (T)(uintptr_t)p; }
constexpr int RX_BIAS = 1 << 15;  // table entries hold t0 + RX_BIAS: the extrapolated texel of a tile's pixel 0 may lie left of / above the image

__device__ __forceinline__ uint32_t sad_u16(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u16(a, b, acc); }

template <int N>
__device__ __forceinline__ void wait_vm()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// planner: per-axis tables
// ------------------------------------------------------------------------------------------------------
// A view is eligible when Tx does not depend on the row, Ty not on the column and w on nothing (and w > 0).
template <typename Q>
__device__ __forceinline__ bool rect_view(Q q) { return q[1] == 0.0f && q[4] == 0.0f && q[8] == 0.0f && q[9] == 0.0f && q[10] == 0.0f && q[11] > 0.0f; }

// 256 r of an eligible view, as sweep_fx_tiled forms it: the w row divided by 256 (exact), s.w = fma(z, 0, q11 / 256) = q11 / 256
template <typename Q>
__device__ __forceinline__ float rect_r256(Q q) { return rcp_rn(q[11] * 0.00390625f); }

// Tx of column c / Ty of row r at plane z: the contract's expression with the terms that vanish left in (fma(0, t, u) = u exactly)
template <typename Q>
__device__ __forceinline__ float rect_tx(Q q, float r256, float z, int c, float invW)
{
    const float xn = __builtin_fmaf((float)(2 * c + 1), invW, -1.0f);
    const float ax = __builtin_fmaf(q[0], xn, __builtin_fmaf(q[1], 0.0f, q[3]));
    return __builtin_fmaf(__builtin_fmaf(z, q[2], ax), r256, RX_MAGIC + 4.0f);
}
template <typename Q>
__device__ __forceinline__ float rect_ty(Q q, float r256, float z, int r, float invH)
{
    const float yn = __builtin_fmaf(-(float)(2 * r + 1), invH, 1.0f);
    const float ay = __builtin_fmaf(q[4], 0.0f, __builtin_fmaf(q[5], yn, q[7]));
    return __builtin_fmaf(__builtin_fmaf(z, q[6], ay), r256, RX_MAGIC + 4.0f);
}

// Table set of one plan (device pointers into ctx->rect_tab).  T = tiles_x resp. tiles_y, NC = plane chunks, dpad = 16 NC.
struct RectTables {
    uint32_t *xt, *yt;    // [T][V][dpad]   full entries (below)
    uint32_t *xmm, *ymm;  // [T][V][dpad]   lowest | highest << 16 integer texel over the tile's in-frame pixels, 0xffffffff if none
    uint32_t *wt;         // [V][dpad]      weight word of the view's nominal phase pair at that plane
    uint32_t *xw;         // [tiles_x][NC][views of the launch][4 wavefronts][16]  X records (pass C)
    uint32_t *yr;         // [tiles_y][NC][views of the launch][4 wavefronts][16]  Y records
    uint32_t *xbox, *ybox;  // [T][V][NC]   region boxes (pass B)
    int *stats;           // [0] widest region (quads), [1] tallest region (rows), [2] planes that are not FULL (diagnostic)
    int dpad;
};

// Pass A.  One thread per (tile column or tile row, view, plane), evaluating every pixel of the tile.  Full entry:
//   bits  0-19  t0 + RX_BIAS, t0 = (u >> 3) - 32 i of the in-frame pixels (i = index in the tile, u = 1/256-texel coordinate):
//               phase in the low 5 bits, integer texel of the tile's pixel 0 (extrapolated, possibly left of the image) above
//   bits 20-26  n = pixels of the tile that are out of frame (all of the tile's pixels: 64 resp. 8)
//   bit  27     which end: 0 = the first n pixels are out, 1 = the last n
//   bit  30     certificate: the out-of-frame pixels are exactly those n, every other pixel has (u >> 3) - 32 i == t0, and
//               the phase is the view's nominal one for this plane (the phase at the image centre: the W table's)
// Pixels past the image edge (ragged last tile) count as matching.
__global__ __launch_bounds__(256) void plan_rect_axis(SweepParams p, RectTables rt, const uint32_t *__restrict__ lut)
{
    const int dpad = rt.dpad;
    const int nx = p.tiles_x * p.V * dpad, ny = p.tiles_y * p.V * dpad, nw = p.V * dpad;
    int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= nx + ny + nw) return;
    const int which = tid < nx ? 0 : (tid < nx + ny ? 1 : 2);
    if (which == 1) tid -= nx;
    if (which == 2) tid -= nx + ny;
    const int d = tid % dpad, v = (tid / dpad) % p.V, t = tid / (dpad * p.V);
    const float *q = p.Q + 12 * v;
    const bool elig = rect_view(q);
    const float r256 = rect_r256(q);
    const float z = p.z[min(d, p.D - 1)];
    const float hix = RX_MAGIC + 132.0f + 256.0f * (float)p.W, hiy = RX_MAGIC + 132.0f + 256.0f * (float)p.H;
    const uint32_t nomx = (__builtin_bit_cast(uint32_t, rect_tx(q, r256, z, p.W / 2, p.invW)) >> 3) & 31u;
    const uint32_t nomy = (__builtin_bit_cast(uint32_t, rect_ty(q, r256, z, p.H / 2, p.invH)) >> 3) & 31u;
    if (which == 2) {
        rt.wt[tid] = lut[nomy * 32u + nomx];
        return;
    }
    const int size = which == 0 ? TILE_W : RX_TILE_H;
    const int first = t * size;
    const int count = min(first + size, which == 0 ? p.W : p.H) - first;  // pixels of the tile inside the image
    int nin = 0, first_in = -1, last_in = -1;
    int t0 = 0;
    uint32_t lo = 0xffffu, hi = 0u;
    bool uniform = elig;
    for (int i = 0; i < count; i++) {
        const float T = which == 0 ? rect_tx(q, r256, z, first + i, p.invW) : rect_ty(q, r256, z, first + i, p.invH);
        if (!(T > RX_MAGIC + 132.0f && T < (which == 0 ? hix : hiy))) continue;
        const uint32_t u = __builtin_bit_cast(uint32_t, T) & 0x3fffffu;
        const int ti = (int)(u >> 3) - 32 * i;
        if (nin == 0) {
            t0 = ti;
            first_in = i;
        }
        uniform = uniform && ti == t0;
        lo = min(lo, u >> 8);
        hi = max(hi, u >> 8);
        last_in = i;
        nin++;
    }
    int nout = size, side = 0;
    if (nin > 0) {
        uniform = uniform && last_in - first_in + 1 == nin;             // contiguous
        if (first_in == 0) {                                            // the tail is out (or nothing: pixels past the image edge are don't-cares)
            side = 1;
            nout = last_in == count - 1 ? 0 : size - 1 - last_in;
        } else {
            side = 0;
            nout = first_in;
            uniform = uniform && last_in == count - 1;                  // cut at both ends: not representable
        }
        uniform = uniform && (uint32_t)(t0 & 31) == (which == 0 ? nomx : nomy) && t0 + RX_BIAS >= 0 && t0 + RX_BIAS < (1 << 20);
    }
    // (no pixel in frame: n = the whole tile and the certificate as computed so far -- nothing to sample)
    (which == 0 ? rt.xt : rt.yt)[tid] = ((uint32_t)(t0 + RX_BIAS) & 0xfffffu) | ((uint32_t)nout << 20) | ((uint32_t)side << 27) | (uniform ? RX_UNIFORM : 0u);
    (which == 0 ? rt.xmm : rt.ymm)[tid] = nin > 0 ? (lo | (hi << 16)) : 0xffffffffu;
}

// Pass B.  One thread per (tile column or tile row, view, chunk): the box of the view's quad image the chunk's 16 planes touch
// (x origin a multiple of 4 quads: the copies move 16-byte units):  box = origin | extent << 16 | any << 31
// (any: some pixel of some plane is in frame).  Counters: widest / tallest box.
__global__ __launch_bounds__(256) void plan_rect_box(SweepParams p, RectTables rt)
{
    const int NC = p.nchunks, dpad = rt.dpad;
    const int nx = p.tiles_x * p.V * NC, ny = p.tiles_y * p.V * NC;
    const bool live = (int)(blockIdx.x * blockDim.x + threadIdx.x) < nx + ny;  // (no early return: the counters are reduced per wavefront)
    int tid = min((int)(blockIdx.x * blockDim.x + threadIdx.x), nx + ny - 1);
    const int which = tid < nx ? 0 : 1;
    if (which == 1) tid -= nx;
    const int chunk = tid % NC, v = (tid / NC) % p.V, t = tid / (NC * p.V);
    const uint32_t *mm = (which == 0 ? rt.xmm : rt.ymm) + ((size_t)t * p.V + v) * dpad + chunk * RX_PC;
    uint32_t lo = 0xffffu, hi = 0u;
    bool any = false;
    for (int k = 0; k < RX_PC; k++) {
        const uint32_t m = mm[k];
        if (m == 0xffffffffu) continue;
        any = true;
        lo = min(lo, m & 0xffffu);
        hi = max(hi, m >> 16);
    }
    const uint32_t org = any ? (which == 0 ? (lo & ~3u) : lo) : 0u;
    const uint32_t ext = any ? hi + 1u - org : 0u;
    // widest / tallest box: one atomic per wavefront (21 000 threads on two addresses took 0.23 ms)
    const int wx = wave_max_i32(live && any && which == 0 ? (int)ext : 0), wy = wave_max_i32(live && any && which == 1 ? (int)ext : 0);
    if ((threadIdx.x & 63) == 0) {
        if (wx) atomicMax(rt.stats + 0, wx);
        if (wy) atomicMax(rt.stats + 1, wy);
    }
    if (live) (which == 0 ? rt.xbox : rt.ybox)[tid] = org | (min(ext, 0x7fffu) << 16) | (any ? 1u << 31 : 0u);
}

// Pass C (after the host has chosen the row stride RS of the LDS slots from pass B's counters, and again whenever a launch walks the
// regions in another order).  One thread per (tile column or tile row, view, chunk, wavefront): that wavefront's record of the region,
// 16 dwords.  The sweep kernel adds the X record of its tile column and the Y record of its tile row LANE BY LANE (one v_add_u32) and
// takes every scalar of a region's turn from the sum with one v_readlane and nothing behind it -- so each dword is either one table's
// alone (the other holds 0 there) or a sum that means something:
//   dword   X record                                      Y record
//   0 - 3   plane k: 4 (ix - x0 + RX_BIAS_X), or bit 14   plane k: 4 RS (iy - y0 + RX_BIAS_Y), or bit 15
//   4       NEXT region: 4 x0                             NEXT region: byte offset of its first row in the quad images
//   5       NEXT region: 4 x0                             NEXT region: that + the bytes its copy spans (below)
//           (a table whose box of the NEXT region is empty: dword 4 = RX_NO_COPY resp. 0, dword 5 = 0 -- the sum ends the copy before its start)
//   6 - 9   weight word of plane k                        0
//   10      1 if any field has the flag or any mask byte is not 0 (both tables: the sum is 0 for a CLEAN region)
//   11      x masks of the four planes                    0
//   12      0                                             y masks of the four planes
//   13      4 x0 | (any ? RS / 4 : 0) << 16               0
//   14      0                                             (any ? rows : 0) | y0 << 8
//   15      0                                             byte offset of THIS region's first row (the workgroup's first copy)
// Plane fields: the plane's share of the LDS byte offset of the texel quad of the tile's pixel 0; the biases because pixel 0 of a tile
// that is partly out of frame lies left of / above the box (the kernel's copies land RX_BIAS bytes into the slot, so base + x share +
// y share is the quad's address; the sum stays below 2^14) -- or a flag (x: bit 14, y: bit 15) = the certificate failed, look at the
// full entry.  A plane whose certificate holds but whose tile is partly (MASKED) or wholly (NONE) out of frame has no flag: its
// out-of-frame pixels come as a mask byte per plane (x: n | side << 7 as in the full entry, n = 64: nothing in frame; y: the bit mask
// of the rows that are OUT of frame), zero for FULL planes.
// NEXT region: a workgroup takes its regions chunks outer, views inner, so the records are laid out in that order
// ([tile][chunk][view of the launch][wavefront], "the next region" = the next 256 bytes) and each carries what the copy of its
// successor needs: the copy is issued a region ahead.  Bytes the copy spans: the kernel's copy instructions have per-lane source
// offsets that grow with the 16-byte unit's index in the box (row-major, RS quads per row), so a buffer that ends
// "4 ((rows - 1) pitch + RS)" bytes behind the box's first quad makes the hardware's range check drop exactly the units past the
// box's last row: no lane mask, no branch.  A workgroup's last region has no NEXT one (RectOrder: the launch's view range, chunk
// range and chunks per workgroup): both tables write it as an empty box.
constexpr int RX_BIAS_X = 64, RX_BIAS_Y = 8;  // quads / rows
constexpr uint32_t RX_NO_COPY = 1u << 24;     // more than any copy spans (32 rows of a 16383-pixel image: 2.1 MB)
constexpr int RX_REC = 16;                    // dwords per record

struct RectOrder {
    int v0, vcount, chunk0, chunk1, cps;
};

__global__ __launch_bounds__(256) void plan_rect_pack(SweepParams p, RectTables rt, int RS, RectOrder o, int count_stats)
{
    const int NC = p.nchunks, dpad = rt.dpad;
    const int nx = p.tiles_x * p.V * NC * 4, ny = p.tiles_y * p.V * NC * 4;
    const bool live = (int)(blockIdx.x * blockDim.x + threadIdx.x) < nx + ny;
    int tid = min((int)(blockIdx.x * blockDim.x + threadIdx.x), nx + ny - 1);
    const int which = tid < nx ? 0 : 1;
    if (which == 1) tid -= nx;
    const int w = tid & 3, chunk = (tid >> 2) % NC, v = ((tid >> 2) / NC) % p.V, t = (tid >> 2) / (NC * p.V);
    const uint32_t *ent = (which == 0 ? rt.xt : rt.yt) + ((size_t)t * p.V + v) * dpad + chunk * RX_PC + w * RX_KW;
    const uint32_t *boxes = which == 0 ? rt.xbox : rt.ybox;
    const uint32_t box = boxes[tid >> 2];
    const int org = (int)(box & 0xffffu), ext = (int)((box >> 16) & 0x7fffu);
    const bool any = (box >> 31) != 0u;
    const int size = which == 0 ? TILE_W : RX_TILE_H;
    uint32_t f[RX_KW], masks = 0u;
    int not_full = 0;
    bool flagged = false;
    for (int k = 0; k < RX_KW; k++) {
        const uint32_t e = ent[k];
        const int tex = ((int)(e & 0xfffffu) - RX_BIAS) >> 5;
        const int nout = (int)((e >> 20) & 127u), side = (int)((e >> 27) & 1u);
        const bool nothing = nout >= size || !any;
        // the in-frame pixels' texels lie inside the box (it is their bounding box); pixel 0's may lie up to `nout` texels before it
        const int bias = which == 0 ? RX_BIAS_X : RX_BIAS_Y;
        const int rel = tex - org + bias;
        const bool certified = (e & RX_UNIFORM) != 0u && (nothing || (rel >= 0 && rel < ext + 2 * bias));
        if (!certified) {
            f[k] = which == 0 ? 0x4000u : 0x8000u;
            flagged = true;
        } else {
            f[k] = nothing ? 0u : (uint32_t)rel * (which == 0 ? 4u : 4u * (uint32_t)RS);
            uint32_t m;
            if (which == 0)
                m = nothing ? 64u : (nout == 0 ? 0u : (uint32_t)nout | ((uint32_t)side << 7));
            else  // rows out of frame: the first `nout` (side 0) or the last `nout` (side 1)
                m = nothing ? 0xffu : (nout == 0 ? 0u : (side ? (0xffu << (RX_TILE_H - nout)) & 0xffu : (1u << nout) - 1u));
            masks |= m << (8 * k);
        }
        not_full += (!certified || ((masks >> (8 * k)) & 0xffu)) ? 1 : 0;
    }
    if (count_stats) {
        const int n = wave_sum_i32(live ? not_full : 0);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(rt.stats + 2, n);
    }
    const int vend = o.v0 + o.vcount;
    if (!live || v < o.v0 || v >= vend) return;
    // the region the workgroup turns to after this one; none after the last region of its share
    const bool last_view = v + 1 == vend;
    const int vn = last_view ? o.v0 : v + 1, cn = last_view ? chunk + 1 : chunk;
    const bool ends = last_view && (chunk < o.chunk0 || chunk + 1 >= o.chunk1 || (chunk + 1 - o.chunk0) % o.cps == 0);
    const uint32_t nbox = ends || cn >= NC ? 0u : boxes[((size_t)t * p.V + vn) * NC + cn];
    const uint32_t norg = nbox & 0xffffu, next = (nbox >> 16) & 0x7fffu;
    const bool nany = (nbox >> 31) != 0u;
    auto first_row = [&](int view, uint32_t y0) {  // (frame-store slot: mvs_sweep_handles)
        return 4u * ((uint32_t)p.pad_slab * (uint32_t)(p.view_slot ? p.view_slot[view] : view) + y0 * (uint32_t)p.pitch);
    };
    const uint32_t clean = (flagged || masks) ? 1u : 0u;
    const size_t slot = (((size_t)t * NC + chunk) * o.vcount + (v - o.v0)) * 4 + w;
    uint32_t *rec = (which == 0 ? rt.xw : rt.yr) + slot * RX_REC;
    for (int k = 0; k < RX_KW; k++) rec[k] = f[k];
    if (which == 0) {
        const uint32_t *wv = rt.wt + (size_t)v * dpad + chunk * RX_PC + w * RX_KW;
        rec[4] = nany ? 4u * norg : RX_NO_COPY;
        rec[5] = nany ? 4u * norg : 0u;
        for (int k = 0; k < RX_KW; k++) rec[6 + k] = wv[k];
        rec[10] = clean;
        rec[11] = masks;
        rec[12] = 0u;
        rec[13] = 4u * (uint32_t)org | ((any ? (uint32_t)RS / 4u : 0u) << 16);
        rec[14] = rec[15] = 0u;
    } else {
        rec[4] = nany ? first_row(vn, norg) : 0u;
        rec[5] = nany ? rec[4] + 4u * ((next - 1u) * (uint32_t)p.pitch + (uint32_t)RS) : 0u;
        rec[6] = rec[7] = rec[8] = rec[9] = 0u;
        rec[10] = clean;
        rec[11] = 0u;
        rec[12] = masks;
        rec[13] = 0u;
        rec[14] = (any ? (uint32_t)ext : 0u) | ((uint32_t)org << 8);
        rec[15] = first_row(v, (uint32_t)org);
    }
}

// ------------------------------------------------------------------------------------------------------
// sweep kernel
// ------------------------------------------------------------------------------------------------------
// What the sweep kernel reads on every region comes in as kernel arguments (SGPRs); what only its rare paths, its prologue and its
// last lines need sits behind one pointer (RectCold, in device memory) and is fetched where it is used: the view loop is short of
// SGPRs, and a spilled SGPR costs vector instructions (v_readlane / v_writelane) in the loop.
struct RectCold {
    const uint8_t *main_img;
    const uint32_t *xt, *yt, *lut;
    const float *Q, *z;
    float *depth, *cost;
    int *index;
    float invW, invH;
    int dpad, v0;  // (v0: the launch's first view -- RectArgs has it too; the failed-certificate block reads it here)
};

struct RectArgs {
    const uint32_t *__restrict__ quads;  // quad images of the side views, pad_slab dwords each
    const uint32_t *__restrict__ xw;
    const uint32_t *__restrict__ yr;
    uint32_t *__restrict__ volume;
    const RectCold *__restrict__ cold;
    uint2 *__restrict__ part;            // plane-split launches: partial bests [gridDim.y][P]
    size_t pad_slab;
    int pitch, W, H, D, V, v0, vcount, nchunks, chunk0, chunk1, cps, ty0, tyn, tiles_x;
    int slot_dw;   // dwords per LDS slot = 256 x copy instructions per region (one instruction fills 256 dwords); two slots
};

template <typename T>
__device__ __forceinline__ T cold_get(uintptr_t c, size_t off)
{
    return *(const __attribute__((address_space(4))) T *)(c + off);
}
#define RX_COLD(c, T, field) cold_get<T>((uintptr_t)(c), offsetof(RectCold, field))

// raw buffer resource over `bytes` bytes at p (gfx950: dword 3 = 0x00020000, 32-bit data format): buffer instructions take a
// wave-uniform resource + a 32-bit per-lane offset + a wave-uniform offset, so no access of the view loop needs a 64-bit per-lane
// address (through plain pointers the compiler forms one for every load, store and LDS copy: 2 VGPRs and 1-2 VALU instructions each).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)bytes, 0x00020000);
}

template <int RS, bool WRITE_VOLUME, bool FUSED>
__global__ __launch_bounds__(256, RX_WAVES_PER_SIMD) void sweep_fx_rect(RectArgs a)
{
    constexpr int UNITS = RS / 4;  // 16-byte units per region row
    constexpr int SLOT_BIAS_DW = RX_BIAS_X + RX_BIAS_Y * RS;  // dwords
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) void *)smem;  // (through a generic pointer: a null check per use)

    const int band_tile = grouped_tile(blockIdx.x, a.tiles_x, a.tyn);
    if (band_tile < 0) return;
    const int tx = band_tile % a.tiles_x, ty = band_tile / a.tiles_x + a.ty0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = tx * TILE_W + lane;
    const int row0 = ty * RX_TILE_H;
    const bool col_ok = col < a.W;
    const int NC = a.nchunks;

    // per-lane source offsets (bytes) of this wavefront's copy instructions: instruction i = wave + 4 t fills LDS dwords
    // [256 i, 256 i + 256) of the slot = 16-byte units g = 64 i + lane of the dense [row][RS] region image.  They grow with g
    // (pitch >= RS), so the units of a region's box are exactly those whose offset lies below the size plan_rect_pack put into the
    // region's record: the copies run through a buffer resource of that size and the range check drops the rest.
    uint32_t srcoff[RX_MAX_NI];
#pragma unroll
    for (int t = 0; t < RX_MAX_NI; t++) {
        const int g = (wave + 4 * t) * 64 + lane;
        srcoff[t] = 4u * (uint32_t)((g / UNITS) * a.pitch + (g % UNITS) * 4);
    }
    uint32_t Im255[8];
    {
        const uint8_t *img = RX_COLD(a.cold, const uint8_t *, main_img);
#pragma unroll
        for (int j = 0; j < 8; j++) Im255[j] = (col_ok && row0 + j < a.H) ? 255u * (uint32_t)img[(size_t)(row0 + j) * a.W + col] : 0u;
    }

    // copy instructions of this wavefront per region: a constant of the launch (the slot holds a.slot_dw / 256 instructions' worth;
    // one more would land in the other slot)
    int ni_wave = (a.slot_dw / 256 + 3 - wave) >> 2;

    const int chunk_first = a.chunk0 + (int)blockIdx.y * a.cps;
    const int chunk_last = min(a.chunk1, chunk_first + a.cps);
    const int nreg = (chunk_last - chunk_first) * a.vcount;

    // this wavefront's records of the workgroup's regions, in the order it takes them (plan_rect_pack): 16 dwords every 256 bytes from
    // `xo` (tile column) and from `xo + ydelta` (tile row); both tables live in one allocation (a.xw < a.yr): one resource, two offsets
    const __amdgpu_buffer_rsrc_t rtab = make_rsrc(a.xw, 0xffffffffu);
    uint32_t xo = (uint32_t)(((((size_t)tx * NC + chunk_first) * a.vcount) * 4 + wave) * (4 * RX_REC));
    const uint32_t ydelta = (uint32_t)((size_t)((const char *)a.yr - (const char *)a.xw) + ((((size_t)ty * NC + chunk_first) * a.vcount) * 4 + wave) * (4 * RX_REC)) - xo;

    // request a region into the slot at LDS byte `slot_b`: src = byte offset of the box's first quad in the quad images (the copies'
    // scalar offset), end = where the copy stops fetching, counted like src from the start of the quad images (the size of the buffer
    // resource the copies go through: gfx950 drops a lane whose offset PLUS the scalar offset reaches it; end <= src: nothing is
    // fetched).  Every wavefront issues all its instructions for every region, whole wavefront, no EXEC write: a lane past the box's
    // last row fetches nothing (the slot has room for it: a.slot_dw counts whole instructions, and no read goes there).
    typedef __attribute__((address_space(3))) char *lds_ptr;
    const uint32_t wrel = 4u * (uint32_t)(SLOT_BIAS_DW + wave * 256);  // where this wavefront's first instruction lands inside a slot
    auto issue_copy = [&](uint32_t src, uint32_t end, uint32_t dst_b) {
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void *)a.quads, 0, (int)end, 0x00020000);
        const lds_ptr dst = (lds_ptr)(uintptr_t)dst_b;
        static_assert(RX_MAX_NI == 3, "the three lines below");
        // (compared where it is used, s_cmp + s_cbranch_scc: or the tests live in SGPR pairs over the whole loop.  The count itself goes
        // through the statement, not a copy of it: one register for the whole loop and no s_mov per turn)
        asm volatile("" : "+s"(ni_wave));
        if (ni_wave >= 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, dst, 16, srcoff[0], src, 0, 0);
        if (ni_wave >= 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, dst + 4096, 16, srcoff[1], src, 0, 0);
        if (ni_wave >= 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, dst + 8192, 16, srcoff[2], src, 0, 0);
    };

    // The records travel through VECTOR registers (lane l holds dword l; one v_readlane per scalar when the region's turn comes): as
    // scalar loads they would have to stay in SGPRs across a whole region's sampling, and the compiler spills them right after the
    // load (a wait for the load, then v_writelane / v_readlane pairs) -- measured: 0.65 ms of loop skeleton.  One region ahead: the
    // record of region r + 1 is in flight while region r is sampled; what the copy of region r + 1 needs is in the record of region r.
    const uint32_t lane16 = 4u * (uint32_t)(lane & (RX_REC - 1));
    auto load_rec = [&](uint32_t o) { return __builtin_amdgcn_raw_buffer_load_b32(rtab, lane16, o, 0); };
    auto rdl = [](uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); };

    uint32_t acc[8][RX_KW];
    uint32_t best[8];
    int bi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        best[j] = 0xffffffffu;  // plain comparison (chunk epilogue); the cross-multiplied one starts from (sum 1, count 0)
        bi[j] = -1;
#pragma unroll
        for (int k = 0; k < RX_KW; k++) acc[j][k] = 0u;
    }
    bool plain = true;    // depth selection: every cell so far carries the same count (see the chunk epilogue)
    uint32_t spacc = 0u;  // per plane of this wavefront (one byte each): views of the current chunk whose plane was NOT counted as a whole

    // prologue: the record of region 0 and, from its own fields, the copy of region 0
    uint32_t yo = xo + ydelta;  // (an offset of its own, stepped like xo: no add between the barrier and the second load)
    uint32_t xl = load_rec(xo), yl = load_rec(yo);
    xo += 4u * 4u * RX_REC;
    yo += 4u * 4u * RX_REC;
    // LDS byte address of the slot being sampled.  The two slots' addresses add up to slot_flip, so the other slot is one subtraction
    // away, and so is where this wavefront's copy into the other slot lands (copy_flip): nothing else is derived per turn.
    const uint32_t slot_flip = 2u * lds_base + 4u * (uint32_t)a.slot_dw, copy_flip = slot_flip + wrel;
    uint32_t slot_cur = lds_base;
    asm volatile("" : "+s"(slot_cur));  // (a scalar from the start: sharing the accumulators' zero would take it, and every M0 after it, through vector registers)
    if (nreg > 0) {
        const uint32_t xsx = rdl(xl, 13), rows = (xsx >> 16) ? rdl(yl, 14) & 0xffu : 0u;
        const uint32_t src = (xsx & 0xffffu) + rdl(yl, 15);
        issue_copy(src, rows ? src + 4u * ((rows - 1u) * (uint32_t)a.pitch + (uint32_t)RS) : 0u, slot_cur + wrel);
    }
    int chunk = chunk_first, vleft = a.vcount;  // views of the chunk still to come, this one included; 0: the chunk's epilogue is pending

    // ---- chunk epilogue ---- (cost volume stores and this wavefront's depth selection over the chunk's four planes of its own)
    // It does NOT run at the end of the turn of the chunk's last view: the stores count in vmcnt like the copies, and the next thing
    // every wavefront does there is wait for vmcnt(0) and the barrier -- 32 write acknowledgements per wavefront with nothing to cover
    // them.  It runs one turn later (vleft == 0 says it is pending), behind the barrier and behind the issue of the next copy, in front
    // of that turn's sampling: the stores then have a whole region's sampling before the next full wait.  The workgroup's last chunk
    // is finished behind the loop.  A macro, not a lambda: through a closure two of bi[] end up in scratch memory.
    //  * W, H: not loop-invariant for the optimiser -- what is derived from them (the rows' offsets, the row tests of a ragged tile in
    //    SGPR pairs) is derived here, once per chunk, not held in SGPRs over the whole region loop.
    //  * pix0: byte offset of this lane's first pixel inside a plane.
    //  * While every plane of every chunk so far was FULL for every view, every cell carries the same count and the packed cells
    //    compare like their sums: "cell < best" (best starts at 0xffffffff) instead of the cross-multiplied comparison.  The first
    //    chunk with a plane that is not FULL ends that for the rest of the workgroup (same packed cells, start value 1).
    //  * cntk: FULL planes -- every cell gets the view's count.  One buffer resource per plane (a volume can exceed the 4 GiB a
    //    resource spans), rows by the wave-uniform offset; nt stores: written once, read by a later kernel.
#define RX_CHUNK_EPILOGUE                                                                                                                                                    \
    int W = a.W, H = a.H;                                                                                                                                                    \
    asm volatile("" : "+s"(W), "+s"(H));                                                                                                                                     \
    const int d0 = chunk * RX_PC + wave * RX_KW;                                                                                                                             \
    const size_t P = (size_t)W * H;                                                                                                                                          \
    const uint32_t pix0 = 4u * (uint32_t)(row0 * W + col);                                                                                                                   \
    const int nrows = min(8, H - row0);                                                                                                                                      \
    if (FUSED && plain && spacc != 0u) {                                                                                                                                     \
        plain = false;                                                                                                                                                       \
    _Pragma("unroll")                                                                                                                                                        \
        for (int j = 0; j < 8; j++) best[j] = bi[j] < 0 ? 1u : best[j];                                                                                                      \
    }                                                                                                                                                                        \
    auto finish = [&](auto checked_rows, auto plain_compare) {                                                                                                               \
    _Pragma("unroll")                                                                                                                                                        \
        for (int k = 0; k < RX_KW; k++) {                                                                                                                                    \
            const uint32_t cntk = ((uint32_t)a.vcount - ((spacc >> (8 * k)) & 0xffu)) << 24;                                                                                 \
            if (d0 + k < a.D) {                                                                                                                                              \
                const __amdgpu_buffer_rsrc_t rvol = make_rsrc(WRITE_VOLUME ? a.volume + (size_t)(d0 + k) * P : nullptr, 0xffffffffu);                                        \
    _Pragma("unroll")                                                                                                                                                        \
                for (int j = 0; j < 8; j++) {                                                                                                                                \
                    if (!checked_rows.value || j < nrows) {                                                                                                                  \
                        const uint32_t cell = acc[j][k] + cntk;                                                                                                              \
                        if (WRITE_VOLUME) __builtin_amdgcn_raw_buffer_store_b32(cell, rvol, pix0, 4u * (uint32_t)(j * W), 2);                                                \
                        if (FUSED) {                                                                                                                                         \
                            const bool better = plain_compare.value ? cell < best[j] : umul24u(cell & 0xffffffu, best[j] >> 24) < umul24u(best[j] & 0xffffffu, cell >> 24);  \
                            best[j] = better ? cell : best[j];                                                                                                               \
                            bi[j] = better ? d0 + k : bi[j];                                                                                                                 \
                        }                                                                                                                                                    \
                    }                                                                                                                                                        \
                }                                                                                                                                                            \
            }                                                                                                                                                                \
        }                                                                                                                                                                    \
    };                                                                                                                                                                       \
    if (col_ok) {                                                                                                                                                            \
        if (nrows == 8 && plain)                                                                                                                                             \
            finish(std::false_type{}, std::true_type{});                                                                                                                     \
        else if (nrows == 8)                                                                                                                                                 \
            finish(std::false_type{}, std::false_type{});                                                                                                                    \
        else if (plain)                                                                                                                                                      \
            finish(std::true_type{}, std::true_type{});                                                                                                                      \
        else                                                                                                                                                                 \
            finish(std::true_type{}, std::false_type{});                                                                                                                     \
    }                                                                                                                                                                        \
    _Pragma("unroll")                                                                                                                                                        \
    for (int k = 0; k < RX_KW; k++)                                                                                                                                          \
    _Pragma("unroll")                                                                                                                                                        \
        for (int j = 0; j < 8; j++) acc[j][k] = 0u;                                                                                                                          \
    spacc = 0u;                                                                                                                                                              \
    vleft = a.vcount;                                                                                                                                                        \
    chunk++;

    for (int r = nreg; r > 0; r--) {
        // every copy and every record this wavefront asked for has landed ...
        wait_vm<0>();
        // ... and so have every other wavefront's; nobody reads region r - 1 any more
        __builtin_amdgcn_s_barrier();
        // this region's scalars, lane by lane (plan_rect_pack): one vector add, then one v_readlane each
        const uint32_t rsum = xl + yl;
        // the record of region r + 1 and the copy of region r + 1 into the other slot (nothing behind a workgroup's last region: its
        // record ends the copy where it starts): in flight during this region's sampling
        xl = load_rec(xo);
        yl = load_rec(yo);
        xo += 4u * 4u * RX_REC;
        yo += 4u * 4u * RX_REC;
        issue_copy(rdl(rsum, 4), rdl(rsum, 5), copy_flip - slot_cur);
        // the previous turn ended a chunk: its epilogue, before this turn's sampling adds to the accumulators and to spacc
        if (__builtin_expect(vleft == 0, 0)) {
            RX_CHUNK_EPILOGUE
        }
        const uint32_t we[RX_KW] = {rdl(rsum, 6), rdl(rsum, 7), rdl(rsum, 8), rdl(rsum, 9)};
        const uint32_t fld[RX_KW] = {rdl(rsum, 0), rdl(rsum, 1), rdl(rsum, 2), rdl(rsum, 3)};  // per plane: LDS byte offset, or a flag bit

        // ---- sample region r ----
        {
            const uint32_t slot_byte = slot_cur;
            uint32_t qd[1][8];
            const uint32_t clean = rdl(rsum, 10);  // 0: CLEAN (no flag in a field, no mask byte)
            {
                // CLEAN region (every plane FULL: certified, every pixel in frame): one straight-line statement for the four planes,
                // no EXEC write, no branch.  The reads of plane k + 1 follow the v_sad_u16s of plane k row by row into the same 8
                // registers (row j's read behind row j's sad), so they are in flight while plane k finishes; plane k + 1's v_dot4s then
                // wait for their pair of rows with a counted lgkmcnt (LDS reads return in order).  The lgkmcnt(0) in front: a scalar
                // load the compiler left in flight would make the counted waits a lower bound only.  Every v_sad reads a v_dot4 result
                // 8 VALU instructions after it was written (the pair needs wait states the compiler does not insert inside asm);
                // the M0 write of the first plane gets its wait state from the s_nop, the later ones from the v_sad in front of the read.
#define RX_RD(j) "ds_read_addtid_b32 %[q" #j "] offset:%[o" #j "]\n\t"
#define RX_DOT(j, k) "v_dot4_u32_u8 %[q" #j "], %[q" #j "], %[w" #k "], 0\n\t"
#define RX_SAD(j, k) "v_sad_u16 %[a" #j #k "], %[q" #j "], %[i" #j "], %[a" #j #k "]\n\t"
#define RX_DOTS(k)                                                                                                        \
    "s_waitcnt lgkmcnt(6)\n\t" RX_DOT(0, k) RX_DOT(1, k) "s_waitcnt lgkmcnt(4)\n\t" RX_DOT(2, k) RX_DOT(3, k)                \
    "s_waitcnt lgkmcnt(2)\n\t" RX_DOT(4, k) RX_DOT(5, k) "s_waitcnt lgkmcnt(0)\n\t" RX_DOT(6, k) RX_DOT(7, k)
#define RX_PLANE(k, kn)                                                                                                   \
    RX_DOTS(k) "s_add_u32 m0, %[slot], %[f" #kn "]\n\t"                                                                  \
    RX_SAD(0, k) RX_RD(0) RX_SAD(1, k) RX_RD(1) RX_SAD(2, k) RX_RD(2) RX_SAD(3, k) RX_RD(3)                                  \
    RX_SAD(4, k) RX_RD(4) RX_SAD(5, k) RX_RD(5) RX_SAD(6, k) RX_RD(6) RX_SAD(7, k) RX_RD(7)
#define RX_ACC(k)                                                                                                         \
    [a0##k] "+v"(acc[0][k]), [a1##k] "+v"(acc[1][k]), [a2##k] "+v"(acc[2][k]), [a3##k] "+v"(acc[3][k]),                   \
    [a4##k] "+v"(acc[4][k]), [a5##k] "+v"(acc[5][k]), [a6##k] "+v"(acc[6][k]), [a7##k] "+v"(acc[7][k])
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
                asm volatile("s_cmp_lg_u32 %[cl], 0\n\t"
                             "s_cbranch_scc1 9f\n\t"
                             "s_waitcnt lgkmcnt(0)\n\t"
                             "s_add_u32 m0, %[slot], %[f0]\n\t"
                             "s_nop 0\n\t"
                             RX_RD(0) RX_RD(1) RX_RD(2) RX_RD(3) RX_RD(4) RX_RD(5) RX_RD(6) RX_RD(7)
                             RX_PLANE(0, 1) RX_PLANE(1, 2) RX_PLANE(2, 3)
                             RX_DOTS(3)
                             RX_SAD(0, 3) RX_SAD(1, 3) RX_SAD(2, 3) RX_SAD(3, 3) RX_SAD(4, 3) RX_SAD(5, 3) RX_SAD(6, 3) RX_SAD(7, 3)
                             "9:"
                             : [q0] "=&v"(qd[0][0]), [q1] "=&v"(qd[0][1]), [q2] "=&v"(qd[0][2]), [q3] "=&v"(qd[0][3]), [q4] "=&v"(qd[0][4]), [q5] "=&v"(qd[0][5]), [q6] "=&v"(qd[0][6]), [q7] "=&v"(qd[0][7]),
                               RX_ACC(0), RX_ACC(1), RX_ACC(2), RX_ACC(3)
                             : [cl] "s"(clean), [slot] "s"(slot_byte), [f0] "s"(fld[0]), [f1] "s"(fld[1]), [f2] "s"(fld[2]), [f3] "s"(fld[3]),
                               [w0] "s"(we[0]), [w1] "s"(we[1]), [w2] "s"(we[2]), [w3] "s"(we[3]),
                               [i0] "v"(Im255[0]), [i1] "v"(Im255[1]), [i2] "v"(Im255[2]), [i3] "v"(Im255[3]), [i4] "v"(Im255[4]), [i5] "v"(Im255[5]), [i6] "v"(Im255[6]), [i7] "v"(Im255[7]),
                               [o0] "n"(0), [o1] "n"(RS * 4), [o2] "n"(RS * 8), [o3] "n"(RS * 12), [o4] "n"(RS * 16), [o5] "n"(RS * 20), [o6] "n"(RS * 24), [o7] "n"(RS * 28)
                             : "m0", "scc");
#pragma clang diagnostic pop
#undef RX_ACC
#undef RX_PLANE
#undef RX_DOTS
#undef RX_SAD
#undef RX_DOT
#undef RX_RD
            }
            if (__builtin_expect(clean != 0u, 0)) {
                const uint32_t special = (fld[0] | fld[1] | fld[2] | fld[3]) & 0xc000u;
                // per plane: what is out of frame although the certificates hold (0: nothing -- with no flag in the field that is a FULL plane)
                const uint32_t xmasks = rdl(rsum, 11), ymasks = rdl(rsum, 12);
                const uint32_t anymask = xmasks | ymasks;
                if (__builtin_expect(anymask != 0u, 0)) {
#pragma unroll
                    for (int k = 0; k < RX_KW; k++)
                        if (((anymask >> (8 * k)) & 0xffu) && !(fld[k] & 0xc000u)) spacc += 1u << (8 * k);  // this view's count does not go to every cell of the plane
                }
                // One asm statement per plane: LDS base in M0 (ds_read_addtid_b32: M0 + offset + 4 lane, no address register), weight word in
                // an SGPR, 8 reads, 8 v_dot4, 8 v_sad_u16 (all dot products before all differences: a v_sad right behind the v_dot4 it
                // consumes costs wait states).  A plane whose certificate failed (flag bits in the field) reads as well (somewhere in or past
                // the LDS: harmless) and runs its vector instructions with EXEC = 0; the block below does those planes.  The s_and between
                // the write of M0 and the first read is the wait state that pair needs.
                // A plane of a tile at the border of the side view (its byte of `am` is not 0) branches to the tail INSIDE the statement --
                // same registers, no second shape for the register allocator: EXEC = the lanes in frame (x byte: n | side << 7, n = 64:
                // none), then row by row EXEC = that or nothing (y byte: the rows that are out), each cell that gets the sample counting it
                // itself (+ 1 << 24).  The tail costs the planes that are FULL one taken s_branch.
#define RX_ROW_TAIL(j)                                                                                                   \
        "s_bitcmp0_b32 %[ym], %[yb" #j "]\n\ts_cselect_b64 exec, vcc, 0\n\tv_add_u32 %[a" #j "], 0x1000000, %[a" #j "]\n\t" \
        "v_sad_u16 %[a" #j "], %[q" #j "], %[i" #j "], %[a" #j "]\n\t"
#pragma unroll
                for (int k = 0; k < RX_KW; k++) {
                    // nothing of the plane in frame (x byte: n = 64, or every row out): no reads, no vector work
                    if ((((xmasks >> (8 * k)) & 0x40u) | (((ymasks >> (8 * k)) & 0xffu) == 0xffu)) != 0u) continue;
                    // (experiment 512 -- every plane sampled twice: the work of 8 planes per wavefront, DESIGN A.5b -- has served and is gone: its
                    // run-time trip count no longer compiles with the immediates below)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
                    asm volatile("s_add_u32 m0, %[slot], %[fld]\n\t"
                                 "s_and_b32 vcc_lo, %[fld], 0xc000\n\t"
                                 "ds_read_addtid_b32 %[q0] offset:%[o0]\n\tds_read_addtid_b32 %[q1] offset:%[o1]\n\tds_read_addtid_b32 %[q2] offset:%[o2]\n\tds_read_addtid_b32 %[q3] offset:%[o3]\n\t"
                                 "ds_read_addtid_b32 %[q4] offset:%[o4]\n\tds_read_addtid_b32 %[q5] offset:%[o5]\n\tds_read_addtid_b32 %[q6] offset:%[o6]\n\tds_read_addtid_b32 %[q7] offset:%[o7]\n\t"
                                 "s_cselect_b64 exec, 0, -1\n\t"
                                 "s_bfe_u32 vcc_lo, %[am], %[kb]\n\t"  // this plane's byte of the masks: SCC = not 0
                                 "s_cbranch_scc1 1f\n\t"
                                 "s_waitcnt lgkmcnt(0)\n\t"
                                 "v_dot4_u32_u8 %[q0], %[q0], %[w], 0\n\tv_dot4_u32_u8 %[q1], %[q1], %[w], 0\n\tv_dot4_u32_u8 %[q2], %[q2], %[w], 0\n\tv_dot4_u32_u8 %[q3], %[q3], %[w], 0\n\t"
                                 "v_dot4_u32_u8 %[q4], %[q4], %[w], 0\n\tv_dot4_u32_u8 %[q5], %[q5], %[w], 0\n\tv_dot4_u32_u8 %[q6], %[q6], %[w], 0\n\tv_dot4_u32_u8 %[q7], %[q7], %[w], 0\n\t"
                                 "v_sad_u16 %[a0], %[q0], %[i0], %[a0]\n\tv_sad_u16 %[a1], %[q1], %[i1], %[a1]\n\tv_sad_u16 %[a2], %[q2], %[i2], %[a2]\n\tv_sad_u16 %[a3], %[q3], %[i3], %[a3]\n\t"
                                 "v_sad_u16 %[a4], %[q4], %[i4], %[a4]\n\tv_sad_u16 %[a5], %[q5], %[i5], %[a5]\n\tv_sad_u16 %[a6], %[q6], %[i6], %[a6]\n\tv_sad_u16 %[a7], %[q7], %[i7], %[a7]\n\t"
                                 "2:\n\t"
                                 "s_mov_b64 exec, -1\n\t"
                                 "s_branch 9f\n\t"
                                 // ---- the tail: lanes in frame from the x byte
                                 "1:\n\t"
                                 "s_bfe_u32 vcc_lo, %[xm], %[nb]\n\t"        // n (6 bits)
                                 "s_bitcmp1_b32 %[xm], %[sb]\n\t"            // side
                                 "s_cbranch_scc1 3f\n\t"
                                 "s_lshl_b64 exec, exec, vcc_lo\n\t"         // the first n lanes are out
                                 "s_branch 4f\n\t"
                                 "3:\n\t"
                                 "s_lshr_b64 exec, exec, vcc_lo\n\t"         // the last n lanes are out
                                 "4:\n\t"
                                 "s_bitcmp1_b32 %[xm], %[eb]\n\t"            // n = 64: nothing in frame
                                 "s_cselect_b64 exec, 0, exec\n\t"
                                 "s_mov_b64 vcc, exec\n\t"
                                 "s_waitcnt lgkmcnt(0)\n\t"
                                 "v_dot4_u32_u8 %[q0], %[q0], %[w], 0\n\tv_dot4_u32_u8 %[q1], %[q1], %[w], 0\n\tv_dot4_u32_u8 %[q2], %[q2], %[w], 0\n\tv_dot4_u32_u8 %[q3], %[q3], %[w], 0\n\t"
                                 "v_dot4_u32_u8 %[q4], %[q4], %[w], 0\n\tv_dot4_u32_u8 %[q5], %[q5], %[w], 0\n\tv_dot4_u32_u8 %[q6], %[q6], %[w], 0\n\tv_dot4_u32_u8 %[q7], %[q7], %[w], 0\n\t"
                                 RX_ROW_TAIL(0) RX_ROW_TAIL(1) RX_ROW_TAIL(2) RX_ROW_TAIL(3) RX_ROW_TAIL(4) RX_ROW_TAIL(5) RX_ROW_TAIL(6) RX_ROW_TAIL(7)
                                 "s_branch 2b\n\t"
                                 "9:"
                                 : [q0] "=&v"(qd[0][0]), [q1] "=&v"(qd[0][1]), [q2] "=&v"(qd[0][2]), [q3] "=&v"(qd[0][3]), [q4] "=&v"(qd[0][4]), [q5] "=&v"(qd[0][5]), [q6] "=&v"(qd[0][6]), [q7] "=&v"(qd[0][7]),
                                   [a0] "+v"(acc[0][k]), [a1] "+v"(acc[1][k]), [a2] "+v"(acc[2][k]), [a3] "+v"(acc[3][k]), [a4] "+v"(acc[4][k]), [a5] "+v"(acc[5][k]), [a6] "+v"(acc[6][k]), [a7] "+v"(acc[7][k])
                                 : [slot] "s"(slot_byte), [fld] "s"(fld[k]), [w] "s"(we[k]), [am] "s"(anymask), [xm] "s"(xmasks), [ym] "s"(ymasks),
                                   [i0] "v"(Im255[0]), [i1] "v"(Im255[1]), [i2] "v"(Im255[2]), [i3] "v"(Im255[3]), [i4] "v"(Im255[4]), [i5] "v"(Im255[5]), [i6] "v"(Im255[6]), [i7] "v"(Im255[7]),
                                   [o0] "n"(0), [o1] "n"(RS * 4), [o2] "n"(RS * 8), [o3] "n"(RS * 12), [o4] "n"(RS * 16), [o5] "n"(RS * 20), [o6] "n"(RS * 24), [o7] "n"(RS * 28),
                                   [kb] "n"(8 * k | (8 << 16)), [nb] "n"(8 * k | (6 << 16)), [sb] "n"(8 * k + 7), [eb] "n"(8 * k + 6),
                                   [yb0] "n"(8 * k + 0), [yb1] "n"(8 * k + 1), [yb2] "n"(8 * k + 2), [yb3] "n"(8 * k + 3), [yb4] "n"(8 * k + 4), [yb5] "n"(8 * k + 5), [yb6] "n"(8 * k + 6), [yb7] "n"(8 * k + 7)
                                 : "m0", "scc", "vcc");
#pragma clang diagnostic pop
                }
#undef RX_ROW_TAIL
                // the planes whose certificate failed (a rounding boundary inside the tile), or whose offsets did not fit the record
                if (special) {
                    uintptr_t coldp = (uintptr_t)a.cold;
                    asm volatile("" : "+s"(coldp));  // not loop-invariant for the optimiser: fetched here, not held in SGPRs over the loop
                    const int dpad = RX_COLD(coldp, int, dpad);
                    const int v = RX_COLD(coldp, int, v0) + a.vcount - vleft;
                    const cu32 xt = as_const<cu32>(RX_COLD(coldp, const uint32_t *, xt) + ((size_t)tx * a.V + v) * dpad + chunk * RX_PC + wave * RX_KW);
                    const cu32 yt = as_const<cu32>(RX_COLD(coldp, const uint32_t *, yt) + ((size_t)ty * a.V + v) * dpad + chunk * RX_PC + wave * RX_KW);
                    const uint32_t xsx = rdl(rsum, 13), yn = rdl(rsum, 14);
                    const int x0 = (int)((xsx & 0xffffu) >> 2), y0 = (int)((yn >> 8) & 0x3fffu);
                    const bool staged = (xsx >> 16) != 0u && (yn & 0xffu) != 0u;
#pragma unroll
                    for (int k = 0; k < RX_KW; k++) {
                        if (!(fld[k] & 0xc000u)) continue;
                        spacc += 1u << (8 * k);  // not FULL: this view's count does not go to every cell of the plane
                        if (!staged) continue;
                        const uint32_t xe = xt[k], ye = yt[k];
                        const int nx = (int)((xe >> 20) & 127u), ny = (int)((ye >> 20) & 127u);
                        if ((xe & ye) & RX_UNIFORM) {
                            if (nx >= TILE_W || ny >= RX_TILE_H) continue;  // nothing in frame
                            // a lane range (from the X entry) and a row range (from the Y entry) are in frame: the fast path under a mask,
                            // the in-frame count per cell
                            const int tx0 = (int)(xe & 0xfffffu) - RX_BIAS, ty0 = (int)(ye & 0xfffffu) - RX_BIAS;
                            const uint32_t addr = 4u * (uint32_t)lane + slot_byte + 4u * (uint32_t)(SLOT_BIAS_DW + ((ty0 >> 5) - y0) * RS + ((tx0 >> 5) - x0));
                            const bool lane_in = ((xe >> 27) & 1u) ? lane < TILE_W - nx : lane >= nx;
                            const int jlo = ((ye >> 27) & 1u) ? 0 : ny, jhi = ((ye >> 27) & 1u) ? RX_TILE_H - ny : RX_TILE_H;
                            if (lane_in) {
#pragma unroll
                                for (int j = 0; j < 8; j++) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(qd[0][j]) : "v"(addr), "n"(j * RS * 4));
                                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qd[0][0]), "+v"(qd[0][1]), "+v"(qd[0][2]), "+v"(qd[0][3]), "+v"(qd[0][4]), "+v"(qd[0][5]), "+v"(qd[0][6]), "+v"(qd[0][7]));
#pragma unroll
                                for (int j = 0; j < 8; j++)
                                    if (j >= jlo && j < jhi) acc[j][k] = sad_u16(__builtin_amdgcn_udot4(qd[0][j], we[k], 0u, false), Im255[j], acc[j][k] + (1u << 24));
                            }
                            continue;
                        }
                        // A certificate failed (a rounding boundary inside the tile: ~0.3 % of the planes on the SURVEY 8d ring): the contract's
                        // expression per lane (columns) and per row, then one pass per group of lanes that share a phase and a texel offset
                        // (usually two groups), each with wave-uniform weights and LDS bases like the fast path.
                        const cf32 q = as_const<cf32>(RX_COLD(coldp, const float *, Q) + 12 * v);
                        const float z = as_const<cf32>(RX_COLD(coldp, const float *, z))[min(chunk * RX_PC + wave * RX_KW + k, a.D - 1)];
                        const float invW = RX_COLD(coldp, float, invW), invH = RX_COLD(coldp, float, invH);
                        const cu32 lut = as_const<cu32>(RX_COLD(coldp, const uint32_t *, lut));
                        const uint32_t lo_bits = __builtin_bit_cast(uint32_t, RX_MAGIC + 132.0f);
                        const uint32_t hix_bits = lo_bits + 256u * (uint32_t)a.W, hiy_bits = lo_bits + 256u * (uint32_t)a.H;  // floats in [2^23, 2^24): ulp 1
                        const float r256 = rect_r256(q);
                        const uint32_t txb = __builtin_bit_cast(uint32_t, rect_tx(q, r256, z, col, invW));
                        const bool inx = col_ok && txb > lo_bits && txb < hix_bits;
                        const int tx3 = (int)((txb & 0x3fffffu) >> 3) - 32 * lane;
                        const uint32_t tyv = __builtin_bit_cast(uint32_t, rect_ty(q, r256, z, row0 + (lane & 7), invH));
                        unsigned long long remaining = __builtin_amdgcn_ballot_w64(inx);
                        while (remaining) {
                            const int t = __builtin_amdgcn_readlane(tx3, (int)__builtin_ctzll(remaining));
                            const bool mine = inx && tx3 == t;
                            remaining &= ~__builtin_amdgcn_ballot_w64(mine);
                            const uint32_t kx = (uint32_t)t & 31u;
                            const int ixrel = (t >> 5) - x0;
#pragma unroll
                            for (int j = 0; j < 8; j++) {
                                const uint32_t tyb = (uint32_t)__builtin_amdgcn_readlane((int)tyv, j);
                                if (tyb > lo_bits && tyb < hiy_bits && row0 + j < a.H) {
                                    const uint32_t uy = tyb & 0x3fffffu;
                                    const uint32_t w = lut[((uy >> 3) & 31u) * 32u + kx];
                                    const uint32_t addr = 4u * (uint32_t)lane + slot_byte + 4u * (uint32_t)(SLOT_BIAS_DW + ((int)(uy >> 8) - y0) * RS + ixrel);
                                    if (mine) {
                                        uint32_t quad;
                                        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(quad) : "v"(addr));
                                        acc[j][k] = sad_u16(__builtin_amdgcn_udot4(quad, w, 0u, false), Im255[j], acc[j][k] + (1u << 24));
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }

        // the chunk's last view: its epilogue is left pending for the next turn (or for the lines behind the loop)
        --vleft;
        slot_cur = slot_flip - slot_cur;
    }

    if (nreg > 0) {  // the workgroup's last chunk: the last turn ended it
        RX_CHUNK_EPILOGUE
    }
#undef RX_CHUNK_EPILOGUE

    // ---- depth selection across the four wavefronts (each holds the best of its own planes): lowest cost, ties -> lowest plane ----
    if (FUSED) {
        wait_vm<0>();     // (the last turn's copy fetched nothing, but it is a copy)
        __syncthreads();  // every copy has landed and every sample loop is done: the slots are free
        uint2 *ex = (uint2 *)smem;  // [wave][row][lane]
#pragma unroll
        for (int j = 0; j < 8; j++) ex[(wave * 8 + j) * 64 + lane] = make_uint2(best[j], (uint32_t)bi[j]);
        __syncthreads();
        const size_t P = (size_t)a.W * a.H;
        float *depth = RX_COLD(a.cold, float *, depth), *cost = RX_COLD(a.cold, float *, cost);
        int *index = RX_COLD(a.cold, int *, index);
        const float *zt = RX_COLD(a.cold, const float *, z);
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const int j = wave * 2 + jj;
            const int row = row0 + j;
            if (col_ok && row < a.H) {
                uint32_t b = 1u;
                int bidx = -1;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const uint2 c = ex[(s * 8 + j) * 64 + lane];
                    if ((int)c.y >= 0) {
                        const uint32_t lhs = umul24u(c.x & 0xffffffu, b >> 24), rhs = umul24u(b & 0xffffffu, c.x >> 24);
                        const bool take = lhs < rhs || (lhs == rhs && bidx >= 0 && (int)c.y < bidx);
                        b = take ? c.x : b;
                        bidx = take ? (int)c.y : bidx;
                    }
                }
                if (bidx < 0) b = 0u;  // no plane had a view in frame: the empty cell, as argmin_update_packed leaves it
                const size_t pix = (size_t)row * a.W + col;
                if (a.part) {
                    a.part[(size_t)blockIdx.y * P + pix] = make_uint2(b, (uint32_t)bidx);
                } else {  // store_best<CS_FIXED>
                    depth[pix] = bidx >= 0 ? zt[bidx] : MVS_BACKGROUND_DEPTH;
                    cost[pix] = bidx >= 0 ? cell_cost<CS_FIXED>(b & 0xffffffu, b >> 24) : __builtin_inff();
                    index[pix] = bidx;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------

bool rect_view_host(const float *q) { return q[1] == 0.0f && q[4] == 0.0f && q[8] == 0.0f && q[9] == 0.0f && q[10] == 0.0f && q[11] > 0.0f; }

struct RectSizes {
    size_t nx, ny, nw, nxw, nyr, nxb, nyb, total;
};

static RectSizes rect_sizes(const SweepParams &q)
{
    RectSizes z;
    const size_t dpad = (size_t)q.nchunks * RX_PC;
    z.nx = (size_t)q.tiles_x * q.V * dpad;
    z.ny = (size_t)q.tiles_y * q.V * dpad;
    z.nw = (size_t)q.V * dpad;
    z.nxb = (size_t)q.tiles_x * q.V * q.nchunks;
    z.nyb = (size_t)q.tiles_y * q.V * q.nchunks;
    z.nxw = z.nxb * 4 * RX_REC;  // (a launch over fewer views packs its records into the front of the same tables)
    z.nyr = z.nyb * 4 * RX_REC;
    z.total = 16 + z.nxw + z.nyr + 2 * z.nx + 2 * z.ny + z.nw + z.nxb + z.nyb + 4 * RX_REC;  // + slack: the last turn's prefetch reads one region past the last Y record
    return z;
}

static void rect_tables(mvs_ctx *ctx, const SweepParams &q, RectTables &rt)
{
    const RectSizes z = rect_sizes(q);
    uint32_t *base = (uint32_t *)ctx->rect_tab.ptr;
    rt.dpad = q.nchunks * RX_PC;
    rt.stats = (int *)base;  // 16 dwords
    rt.xw = base + 16;
    rt.yr = rt.xw + z.nxw;
    rt.xt = rt.yr + z.nyr;
    rt.yt = rt.xt + z.nx;
    rt.wt = rt.yt + z.ny;
    rt.xmm = rt.wt + z.nw;
    rt.ymm = rt.xmm + z.nx;
    rt.xbox = rt.ymm + z.ny;
    rt.ybox = rt.xbox + z.nxb;
}

static size_t rect_table_dwords(const SweepParams &q) { return rect_sizes(q).total; }

// Builds the tables for the current (views, planes) and decides whether the rectified kernel serves this plan: every view
// eligible (host check on the f32 view matrices) and every region box within a slot shape the kernel is compiled for (counters of
// pass B: one stream synchronisation per plan).  Called from sweep_fx_plan.
int sweep_rect_plan(mvs_ctx *ctx, PlanHook *between)
{
    struct RunHookOnce {  // whichever way this function leaves, the caller's work has been queued exactly once
        PlanHook *h;
        int rc = MVS_OK;
        bool done = false;
        int go()
        {
            if (!done && h) rc = h->run();
            done = true;
            return rc;
        }
    } hook{between};
    ctx->rect_ok = false;
    ctx->rect_cold_sent = false;  // the tables (and the cold block behind them) may move
    if (ctx->hooks.no_rect) return hook.go();
    if (ctx->V == 0) return hook.go();
    for (int v = 0; v < ctx->V; v++)
        if (!rect_view_host(ctx->q_host.data() + 12 * v)) return hook.go();  // a view that is not rectified: the general kernel
    // the kernel addresses the quad images through one buffer resource with 32-bit byte offsets
    if ((unsigned long long)ctx->pad_slab * (unsigned long long)(ctx->views_in_store ? ctx->store_cap : ctx->V) * 4ull >= (1ull << 32)) return hook.go();
    SweepParams q;
    fill_params(ctx, q, 0, ctx->V, RX_TILE_H, RX_PC);
    int rc;
    if ((rc = ensure(ctx, ctx->rect_tab, rect_table_dwords(q) * sizeof(uint32_t) + sizeof(RectCold) + 256)) || (rc = ensure_fx_lut(ctx))) {
        (void)hook.go();
        return rc;
    }
    if (!ctx->plan_event) MVS_HIP(ctx, hipEventCreateWithFlags(&ctx->plan_event, hipEventDisableTiming));
    RectTables rt;
    rect_tables(ctx, q, rt);
    MVS_HIP(ctx, hipMemsetAsync(rt.stats, 0, 64, ctx->stream));
    const size_t na = (size_t)(q.tiles_x + q.tiles_y + 1) * q.V * rt.dpad;
    plan_rect_axis<<<(unsigned)((na + 255) / 256), 256, 0, ctx->stream>>>(q, rt, (const uint32_t *)ctx->fx_lut.ptr);
    const size_t nb = (size_t)(q.tiles_x + q.tiles_y) * q.V * q.nchunks;
    plan_rect_box<<<(unsigned)((nb + 255) / 256), 256, 0, ctx->stream>>>(q, rt);
    MVS_HIP(ctx, hipGetLastError());
    int stats[4] = {0, 0, 0, 0};
    MVS_HIP(ctx, hipMemcpyAsync(stats, rt.stats, sizeof(stats), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipEventRecord(ctx->plan_event, ctx->stream));
    // the caller's work (quad images of the new views) goes into the queue NOW: it runs while the host waits for the counters
    if ((rc = hook.go())) return rc;
    MVS_HIP(ctx, hipEventSynchronize(ctx->plan_event));
    const int max_rw = stats[0], max_rh = stats[1];
    int rs = 0;
    if (ctx->hooks.rect_verbose) fprintf(stderr, "sweep_rect_plan: widest box %d quads, tallest %d rows\n", max_rw, max_rh);
    for (int cand : {64, 84, 96, 128})  // row strides the kernel is compiled for
        if (max_rw <= cand) {
            rs = cand;
            break;
        }
    if (!rs || max_rw <= 0 || max_rh <= 0 || max_rh > 32) return MVS_OK;  // wide baselines / few planes: boxes too large for the slots
    const int units = rs / 4;
    const int instrs = div_up(max_rh * units, 64);  // 1 KiB copy instructions per region
    if (instrs > 4 * RX_MAX_NI || instrs * 1024 >= 16384) return MVS_OK;
    if (4 * (rs + RX_BIAS_X) + 4 * rs * (max_rh + RX_BIAS_Y) >= 16384) return MVS_OK;  // the records hold 14-bit (biased) LDS offsets
    ctx->rect_rs = rs;
    ctx->rect_slot_dw = instrs * 256;
    ctx->rect_dpad = rt.dpad;
    // the records in the order of a launch over all views and all chunks, one workgroup per tile (sweep_rect_launch packs them again
    // for the order it walks them in, if that is another)
    const RectOrder order = {0, q.V, 0, q.nchunks, q.nchunks};
    plan_rect_pack<<<(unsigned)((4 * nb + 255) / 256), 256, 0, ctx->stream>>>(q, rt, rs, order, 1);
    MVS_HIP(ctx, hipGetLastError());
    ctx->rect_order = {order.v0, order.vcount, order.chunk0, order.chunk1, order.cps};
    if (ctx->hooks.rect_verbose) {
        // which region bodies the sweep kernel will run.  CLEAN regions (tile, chunk, view, wavefront): no flag in the four fields and
        // no mask byte, in the X record of the tile column and in the Y record of the tile row.  Per (region, plane) of the others:
        // nothing in frame (x byte n = 64 or y byte 0xff in either record: the plane is branched over), a failed certificate (a flag
        // in either record: the cold block), and the border planes by the side that is out of frame (left / right / top / bottom).
        const RectSizes z = rect_sizes(q);
        std::vector<uint32_t> xw(z.nxw), yr(z.nyr);
        MVS_HIP(ctx, hipMemcpyAsync(xw.data(), rt.xw, z.nxw * 4, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(ctx, hipMemcpyAsync(yr.data(), rt.yr, z.nyr * 4, hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const size_t per = (size_t)q.V * q.nchunks * 4;  // records per tile column / tile row (the same order in both tables)
        const double TX = q.tiles_x, TY = q.tiles_y;
        double clean = 0.0, none = 0.0, flagged = 0.0, side[4] = {0.0, 0.0, 0.0, 0.0};
        for (size_t e = 0; e < per; e++) {
            size_t cx = 0, cy = 0;
            for (int t = 0; t < q.tiles_x; t++) {
                const uint32_t *r = xw.data() + ((size_t)t * per + e) * RX_REC;
                cx += r[10] == 0u;
            }
            for (int t = 0; t < q.tiles_y; t++) {
                const uint32_t *r = yr.data() + ((size_t)t * per + e) * RX_REC;
                cy += r[10] == 0u;
            }
            clean += (double)cx * (double)cy;
            for (int k = 0; k < RX_KW; k++) {
                double xn = 0, xf = 0, yn = 0, yf = 0, l = 0, rt_ = 0, tp = 0, bt = 0;
                for (int t = 0; t < q.tiles_x; t++) {
                    const uint32_t *r = xw.data() + ((size_t)t * per + e) * RX_REC;
                    const uint32_t f = r[k], m = (r[11] >> (8 * k)) & 0xffu;
                    xf += (f & 0x4000u) != 0u;
                    xn += (m & 0x40u) != 0u;
                    l += m != 0u && !(m & 0x40u) && !(m & 0x80u);
                    rt_ += m != 0u && !(m & 0x40u) && (m & 0x80u);
                }
                for (int t = 0; t < q.tiles_y; t++) {
                    const uint32_t *r = yr.data() + ((size_t)t * per + e) * RX_REC;
                    const uint32_t f = r[k], m = (r[12] >> (8 * k)) & 0xffu;
                    yf += (f & 0x8000u) != 0u;
                    yn += m == 0xffu;
                    tp += m != 0u && m != 0xffu && (m & 1u);
                    bt += m != 0u && m != 0xffu && (m & 0x80u);
                }
                none += TX * TY - (TX - xn) * (TY - yn);
                flagged += TX * TY - (TX - xf) * (TY - yf);
                side[0] += l * TY;
                side[1] += rt_ * TY;
                side[2] += tp * TX;
                side[3] += bt * TX;
            }
        }
        // the copies: instructions per region (all four wavefronts' / the most one wavefront issues) and, over the boxes that are not
        // empty, how many lanes of a box's last instruction fetch something (the others are dropped by the range check; 64 = all)
        int live_lo = 65, live_hi = 0, inst_lo = 1 << 30, inst_hi = 0;
        unsigned long long live_set = 0ull;  // bit l - 1: some box's last instruction has l lanes that fetch
        for (size_t e = 0; e < (size_t)q.tiles_y * per; e += 4) {
            const int rows = (int)(yr[e * RX_REC + 14] & 0xffu), n = rows * units;
            if (!rows) continue;
            const int live = n % 64 ? n % 64 : 64;
            live_set |= 1ull << (live - 1);
            live_lo = live < live_lo ? live : live_lo;
            live_hi = live > live_hi ? live : live_hi;
            inst_lo = div_up(n, 64) < inst_lo ? div_up(n, 64) : inst_lo;
            inst_hi = div_up(n, 64) > inst_hi ? div_up(n, 64) : inst_hi;
        }
        fprintf(stderr, "sweep_rect_plan: copies: row stride %d, %d instructions per region (%d per wavefront); boxes need %d to %d, "
                "last instruction %d to %d lanes (set 0x%016llx)\n", rs, instrs, div_up(instrs, 4), inst_lo, inst_hi, live_lo, live_hi, live_set);
        const double nreg = (double)per * TX * TY, npl = nreg * RX_KW;
        fprintf(stderr, "sweep_rect_plan: clean regions %.2f %% of %.0f; planes: nothing in frame %.3f %%, failed certificate %.3f %%, "
                "border left %.3f %% right %.3f %% top %.3f %% bottom %.3f %%\n", 100.0 * clean / nreg, nreg, 100.0 * none / npl,
                100.0 * flagged / npl, 100.0 * side[0] / npl, 100.0 * side[1] / npl, 100.0 * side[2] / npl, 100.0 * side[3] / npl);
    }
    // the cold block (device memory, after the tables)
    RectCold cold;
    cold.main_img = main_image_ptr(ctx);
    cold.xt = rt.xt;
    cold.yt = rt.yt;
    cold.lut = (const uint32_t *)ctx->fx_lut.ptr;
    cold.Q = (const float *)ctx->qmats.ptr;
    cold.z = (const float *)ctx->ztab.ptr;
    cold.depth = (float *)ctx->depth.ptr;
    cold.cost = (float *)ctx->cost.ptr;
    cold.index = (int *)ctx->index.ptr;
    cold.invW = q.invW;
    cold.invH = q.invH;
    cold.dpad = rt.dpad;
    cold.v0 = 0;
    ctx->rect_cold_host.resize(sizeof(RectCold));
    memcpy(ctx->rect_cold_host.data(), &cold, sizeof(RectCold));
    ctx->rect_ok = true;
    return MVS_OK;
}

template <int RS>
static int launch_rect(mvs_ctx *ctx, const RectArgs &a, dim3 grid, size_t lds, const SweepFlags &f)
{
    return with_outputs(f.vol, f.fused, [&](auto vol, auto fused) -> int {
        const auto kernel = sweep_fx_rect<RS, decltype(vol)::value, decltype(fused)::value>;
        MVS_HIP(ctx, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kernel<<<grid, 256, lds, ctx->stream>>>(a);
        MVS_HIP(ctx, hipGetLastError());
        return MVS_OK;
    });
}

// launch of the rectified sweep; `p` carries the plane / row / view ranges
int sweep_rect_launch(mvs_ctx *ctx, SweepParams &p, const SweepFlags &f)
{
    RectTables rt;
    rect_tables(ctx, p, rt);
    // the cold block follows the tables; its output pointers can change between plan and launch (sweep_outputs): re-sent when they do
    RectCold *cold_dev = (RectCold *)((uint32_t *)ctx->rect_tab.ptr + rect_table_dwords(p));
    RectCold cold;
    memcpy(&cold, ctx->rect_cold_host.data(), sizeof(RectCold));
    cold.main_img = main_image_ptr(ctx);
    cold.depth = (float *)ctx->depth.ptr;
    cold.cost = (float *)ctx->cost.ptr;
    cold.index = (int *)ctx->index.ptr;
    cold.v0 = p.v0;
    if (!ctx->rect_cold_sent || memcmp(&cold, ctx->rect_cold_host.data(), sizeof(RectCold)) != 0) {
        memcpy(ctx->rect_cold_host.data(), &cold, sizeof(RectCold));
        MVS_HIP(ctx, hipMemcpyAsync(cold_dev, ctx->rect_cold_host.data(), sizeof(RectCold), hipMemcpyHostToDevice, ctx->stream));
        ctx->rect_cold_sent = true;
    }
    RectArgs a;
    a.quads = p.quads;
    a.xw = rt.xw;
    a.yr = rt.yr;
    a.volume = p.volume;
    a.cold = cold_dev;
    a.part = nullptr;
    a.pad_slab = p.pad_slab;
    a.pitch = p.pitch;
    a.W = p.W;
    a.H = p.H;
    a.D = p.D;
    a.V = p.V;
    a.v0 = p.v0;
    a.vcount = p.vcount;
    a.nchunks = p.nchunks;
    a.chunk0 = p.chunk0;
    a.chunk1 = p.chunk1;
    a.ty0 = p.ty0;
    a.tyn = p.tyn;
    a.tiles_x = p.tiles_x;
    a.slot_dw = ctx->rect_slot_dw;
    size_t lds = ((size_t)2 * a.slot_dw + RX_BIAS_X + (size_t)RX_BIAS_Y * ctx->rect_rs) * 4;  // two slots, the second one's data ends a bias further on
    if (f.fused) lds = lds < 16384 ? 16384 : lds;  // the cross-wavefront depth selection borrows 16 KiB
    if (lds > 160 * 1024) return fail(ctx, MVS_EINVAL, "sweep_rect_launch: %zu bytes of LDS", lds);

    const int groups = div_up(p.tiles_x, 2) * div_up(p.tyn, 4);
    // (the buffer of the partial bests may be allocated here, ahead of the pack launch below: both are ordered on the stream)
    int rc = choose_split(ctx, p, p.tiles_x * p.tyn, 16, f);
    if (rc) return rc;
    a.cps = p.cps;
    a.part = p.part;
    // the records in the order this launch's workgroups walk them (plan_rect_pack); kept until a launch asks for another
    const std::array<int, 5> order = {p.v0, p.vcount, p.chunk0, p.chunk1, p.cps};
    if (order != ctx->rect_order) {
        const size_t nb = (size_t)(p.tiles_x + p.tiles_y) * p.V * p.nchunks;
        plan_rect_pack<<<(unsigned)((4 * nb + 255) / 256), 256, 0, ctx->stream>>>(p, rt, ctx->rect_rs, RectOrder{p.v0, p.vcount, p.chunk0, p.chunk1, p.cps}, 0);
        MVS_HIP(ctx, hipGetLastError());
        ctx->rect_order = order;
    }
    const dim3 grid((unsigned)(div_up(groups, 8) * 64), (unsigned)split_count(p));
    return ctx->rect_rs == 64 ? launch_rect<64>(ctx, a, grid, lds, f) : ctx->rect_rs == 84 ? launch_rect<84>(ctx, a, grid, lds, f)
         : ctx->rect_rs == 96 ? launch_rect<96>(ctx, a, grid, lds, f) : launch_rect<128>(ctx, a, grid, lds, f);
}

}  // namespace mvs
