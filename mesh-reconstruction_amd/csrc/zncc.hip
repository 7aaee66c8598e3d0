// zncc.hip -- ZNCC sweep: zero-mean normalised cross-correlation over a support window as the matching cost of the fixed sampler's sweep
// (DESIGN.md section 21 is the arithmetic contract; tests/zncc_mirror.py states it with integer arrays).
//
// For pixel p, plane d and view v the cost compares the main image A with the warped frame B = (dot + 127) / 255 over the (2 R + 1)^2 window
// around p, taking the pixels of the frame whose own sample is in the view's frame.  The six window sums are exact integers; the last
// steps (a product, a square root, a quotient, a clamp, a scale) are f32, one rounding each.  The volume is the packed volume of the
// ordinary sweep (cells count << 24 | sum, [D][H][W]) with c = floor(32512 (1 - ncc)) in place of |dot - 255 I_main|, so everything behind
// the volume runs on it unchanged.
//
// sweep_fx_zncc<R>: a workgroup is a 32 x 16-pixel tile, 256 threads, two pixels per thread (rows ty and ty + 8 of the tile).  Per
// (plane, view) the threads sample tile + halo once, (32 + 2R)(16 + 2R) samples, band.hip's un-tiled sample with one dword gather per quad
// and the weight table in LDS, and write each as ONE 16-byte element whose fields are wide enough for the whole window:
//   x = a | b << 16        (Sa, Sb <= 81 * 255 < 2^15)
//   y = a b | 1 << 24      (Sab <= 81 * 65025 < 2^23; N <= 81 < 2^7)
//   z = a a,  w = b b      (Saa, Sbb < 2^23)
// or zero for a sample that is out of frame (either frame).  The window sum is then separable with plain uint4 adds and no unpacking:
// a horizontal pass (2R + 1 ds_read_b128 per output, (16 + 2R) x 32 outputs) and a vertical one (2R + 1 per pixel); a wavefront reads 64
// consecutive 16-byte elements, which is conflict free.  Two barriers per (plane, view): samples -> row sums -> pixels; the next
// iteration's sample writes come behind the second barrier and its row-sum writes behind its own first, so neither buffer is doubled.
// Barriers are hidden by the other workgroups of the CU (LDS: 4 KiB table + 16 B (HH HW + 32 HH) = 22.6 / 25.3 / 28.1 / 31.0 KiB at
// R = 1 .. 4), not by a pipeline inside the workgroup.  The view's affine part of the thread's sample positions is amortised over a chunk
// of ZN_PC planes, whose cells live in registers until the chunk's epilogue.
#include "sweep_shared.hpp"

namespace mvs {

namespace {

// (the tile's constants, ZnShape, zncc_sample and zncc_cell are sweep_shared.hpp's: bestk.hip shares them)
template <int R, bool WRITE_VOLUME, bool FUSED>
__global__ __launch_bounds__(ZN_THREADS) void sweep_fx_zncc(SweepParams p, const uint32_t *__restrict__ lut_g)
{
    using S = ZnShape<R>;
    __shared__ uint32_t lut[1024];
    __shared__ uint4 smp[S::SAMPLES];    // [HH][HW] window elements of the current (plane, view)
    __shared__ uint4 rows[S::ROWSUMS];   // [HH][32] horizontal sums
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; i++) lut[tid + ZN_THREADS * i] = lut_g[tid + ZN_THREADS * i];
    __syncthreads();
    const int x0 = blockIdx.x * ZN_TW, y0 = blockIdx.y * ZN_TH;
    // this thread's sample positions: elements tid + 256 s of tile + halo
    float sxn[S::NS], syn[S::NS];
    uint32_t sa[S::NS], saa[S::NS];
#pragma unroll
    for (int s = 0; s < S::NS; s++) {
        const int i = tid + ZN_THREADS * s;
        const int hy = i / S::HW, hx = i - hy * S::HW;
        const int col = x0 - R + hx, row = y0 - R + hy;
        const bool live = i < S::SAMPLES && col >= 0 && col < p.W && row >= 0 && row < p.H;   // rule 2: pixels outside the frame are no members
        sa[s] = live ? (uint32_t)p.main_img[(size_t)row * p.W + col] : 0u;
        saa[s] = sa[s] * sa[s];
        sxn[s] = live ? __builtin_fmaf((float)(2 * col + 1), p.invW, -1.0f) : __builtin_nanf("");
        syn[s] = __builtin_fmaf(-(float)(2 * row + 1), p.invH, 1.0f);
    }
    const int c = tid & (ZN_TW - 1), ty = tid / ZN_TW;   // pixels (c, ty) and (c, ty + 8) of the tile
    const int col = x0 + c;
    const size_t P = (size_t)p.W * p.H;
    const float hix = ZN_MAGIC + 132.0f + 256.0f * (float)p.W, hiy = ZN_MAGIC + 132.0f + 256.0f * (float)p.H;
    uint32_t best[2] = {0u, 0u};
    int bi[2] = {-1, -1};
    for (int d0 = 0; d0 < p.D; d0 += ZN_PC) {
        const int n = min(ZN_PC, p.D - d0);   // (uniform: the barriers below are reached by every thread or by none)
        uint32_t acc[2][ZN_PC];
#pragma unroll
        for (int k = 0; k < ZN_PC; k++) acc[0][k] = acc[1][k] = 0u;
        for (int v = p.v0; v < p.v0 + p.vcount; v++) {
            const float *q = p.Q + 12 * v;
            Affine A[S::NS];
#pragma unroll
            for (int s = 0; s < S::NS; s++) A[s] = view_affine(q, sxn[s], syn[s]);
            const uint32_t *qv = p.quads + p.pad_slab * (size_t)(p.view_slot ? p.view_slot[v] : v);
#pragma unroll
            for (int k = 0; k < ZN_PC; k++) {
                if (k >= n) break;
                const float z = p.z[d0 + k];
#pragma unroll
                for (int s = 0; s < S::NS; s++) {
                    const int i = tid + ZN_THREADS * s;
                    const uint4 e = zncc_sample(A[s], q[2], q[6], q[10], z, qv, (uint32_t)p.pitch, hix, hiy, lut, sa[s], saa[s]);
                    if (i < S::SAMPLES) smp[i] = e;
                }
                __syncthreads();
#pragma unroll
                for (int t = 0; t < S::NR; t++) {
                    const int j = tid + ZN_THREADS * t;   // row sum (hy, cc) = (j / 32, j % 32): elements cc .. cc + 2R of row hy
                    if (j < S::ROWSUMS) {
                        const uint4 *src = smp + (j / ZN_TW) * S::HW + (j & (ZN_TW - 1));
                        uint4 sum = src[0];
#pragma unroll
                        for (int e = 1; e <= 2 * R; e++) sum = add4(sum, src[e]);
                        rows[j] = sum;
                    }
                }
                // ok(p) of the thread's own pixels: read here, the samples are rewritten behind the next barrier
                const uint32_t ok0 = smp[(ty + R) * S::HW + c + R].y >> 24, ok1 = smp[(ty + 8 + R) * S::HW + c + R].y >> 24;
                __syncthreads();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint4 *src = rows + (ty + 8 * h) * ZN_TW + c;   // rows ty + 8h .. + 2R of the halo = the window of tile row ty + 8h
                    uint4 sum = src[0];
#pragma unroll
                    for (int e = 1; e <= 2 * R; e++) sum = add4(sum, src[e * ZN_TW]);
                    acc[h][k] += zncc_cell(sum, h ? ok1 : ok0);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int row = y0 + ty + 8 * h;
            if (col < p.W && row < p.H) {
                const size_t pix = (size_t)row * p.W + col;
#pragma unroll
                for (int k = 0; k < ZN_PC; k++)
                    if (k < n) {
                        if (WRITE_VOLUME) __builtin_nontemporal_store(acc[h][k], p.volume + (size_t)(d0 + k) * P + pix);  // written once, read by a later kernel
                        if (FUSED) argmin_update_packed<CS_FIXED>(acc[h][k], d0 + k, best[h], bi[h]);
                    }
            }
        }
    }
    if (FUSED) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int row = y0 + ty + 8 * h;
            if (col < p.W && row < p.H) store_best<CS_FIXED>(p, (size_t)row * p.W + col, best[h] & 0xffffffu, best[h] >> 24, bi[h]);
        }
    }
}

template <int R>
void zncc_launch(mvs_ctx *ctx, const SweepParams &p, bool vol, bool fused)
{
    const dim3 grid((unsigned)div_up(ctx->W, ZN_TW), (unsigned)div_up(ctx->H, ZN_TH));
    const uint32_t *lut = (const uint32_t *)ctx->fx_lut.ptr;
    with_outputs(vol, fused, [&](auto v, auto f) { sweep_fx_zncc<R, decltype(v)::value, decltype(f)::value><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut); });
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_run_zncc(mvs_ctx *ctx, int view_first, int view_count, int radius, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_run_zncc: null context");
    if (radius < 1 || radius > 4) return fail(ctx, MVS_EINVAL, "mvs_sweep_run_zncc: radius %d outside 1..4", radius);
    return fx_sweep_run(ctx, {"mvs_sweep_run_zncc", view_first, view_count, flags, nullptr, ZN_TH, ZN_PC},
                        [&](const SweepParams &p, const uint32_t *, const float *, bool vol, bool fused) {
                            switch (radius) {
                            case 1: zncc_launch<1>(ctx, p, vol, fused); break;
                            case 2: zncc_launch<2>(ctx, p, vol, fused); break;
                            case 3: zncc_launch<3>(ctx, p, vol, fused); break;
                            default: zncc_launch<4>(ctx, p, vol, fused); break;
                            }
                        });
}
