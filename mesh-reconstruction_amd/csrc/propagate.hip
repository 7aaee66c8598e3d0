// propagate.hip -- hypothesis propagation: PatchMatch refinement of a depth map (DESIGN.md section 25 is the contract;
// tests/propagate_mirror.py states it in numpy float32 and integer arrays).
//
// Every pixel holds a hypothesis (z, gx, gy) -- the NDC depth at its centre and its change per column and per row, a slanted plane -- and
// the packed cell k << 24 | sum (section 22) of that hypothesis.  An iteration is two checkerboard half-passes; an active pixel tests the
// planes of its neighbours at distance 1 and 5 extended to its own position, then `nrandom` perturbations of what it holds by then, and
// keeps whatever is better by the rule of the depth selection (strict, so ties keep the earlier one).  Neighbours at odd Manhattan
// distance are inactive in the half-pass, so it runs in place without a race.  The per-view windowed cost is section 22's on the fixed
// sampler, with window member q of pixel p sampled at z + gx dc + gy dr; no plane table and no D x H x W volume exist.
//
// propagate_pass<COST, R, KMAX>: a 32 x 16 tile per workgroup, 256 threads, one ACTIVE pixel per thread (col = 2 j + ((row + h) & 1)), so
// all lanes work in a checkerboard pass; the init pass is the same kernel with both colours (two pixels per thread, one after the other)
// and the pixel's own hypothesis as its only candidate.  The main image of tile + halo sits in LDS.  Per candidate the thread loops over
// views and window members, adds the window element of zncc_sample / absdiff_sample in registers (no sums are shared between pixels:
// every pixel has its own plane) and merges the views through BkList<KMAX>.  A member's affine part is computed per member (six FMAs;
// staging it per view in LDS was not tried).  One candidate loop with one call site keeps the code of an instantiation at one window
// loop, and the two window loops are NOT unrolled: unrolled, the samples' frame-test masks of a whole window row are live at once and
// every instantiation with a window spilled 3 to 79 scalar registers (ZNCC at radius 2 took 230 vector registers); as loops none
// spills and the vector registers stay at 54 to 78.  36 instantiations as in bestk.hip.
// The guide gate of DESIGN.md section 26 (mvs_propagate_set_gate) is two kernel arguments, not a template parameter: a member is live only
// if its guide value is within tau of the centre's, read from a second byte tile in LDS (the main image again, or the stage's copy of the
// caller's guide); tau = 255, the default, passes every member, so an ungated run computes what it computed without the gate.
// The geometric term of DESIGN.md section 27 (mvs_propagate_set_consistency) is runtime arguments too: a candidate that has a counted view
// is carried through the main camera's inverse into each listed neighbour of the depth store, takes the depth the neighbour's map holds
// at the nearest pixel, comes back, and pays for the distance in pixels between where it left and where it returns (prop_consistency:
// fusion's arithmetic, one gather per neighbour, the matrices read with wave-uniform addresses from the stage's table).  The number of
// neighbours that answer travels with the hypothesis: a candidate that wins brings its count along, a pixel that keeps what it holds
// keeps the byte the map has for it, so the support map is that of the held hypotheses after every launch at one evaluation per
// candidate and none for the kept one.  With no neighbour listed the term is one wave-uniform branch per candidate.
#include "bestk_rules.hpp"
#include "depth_rules.hpp"

#include <cmath>

namespace mvs {

namespace {

constexpr int PR_KEPT = 0, PR_NEAR = 1, PR_FAR = 2, PR_RANDOM = 3;

struct PropArgs {
    float *z, *gx, *gy;              // the hypotheses, H*W each (read and written in place)
    uint32_t *cells;                 // their packed cells
    float *cost;                     // the cells as mean costs (+inf for cell 0)
    unsigned long long *counters;    // kept, near, far, random
    int keep;
    int half;                        // 0 / 1: the half-pass; -1: the init pass
    int nrandom;
    float dz, dg;                    // the random steps of this iteration
    uint32_t seed;                   // mix(seed + (2 t + h))
    int tau;                         // the gate of section 26: member q of p is live only if |G(q) - G(p)| <= tau (255: no gate)
    const uint8_t *guide;            // G, H*W; null: the main image
    // the geometric term of section 27 (nslots = 0: none)
    int nslots;
    const PropGeo *geo;              // the term's table (mvs_internal.hpp); the support map, H*W u8, lies H*W bytes behind the cost map's end
};

// What the kernel needs rarely -- the random candidates' steps and seed, the counters' address at its end -- waits in LDS, not in scalar
// registers held through the window loops: with eight list entries (KMAX = 8) the kernel has none to spare
struct PropCold {
    float dz, dg;
    uint32_t seed, pad;
    unsigned long long *counters;
};

constexpr int PROP_MAX_SLOTS = 8;
constexpr int PROP_GEO_WORDS = sizeof(PropGeo) / 4;

// where the table sits in the stage's allocation: behind the five maps, the guide bytes and the support bytes, on a 16-byte boundary
inline size_t prop_table_at(size_t bytes_before) { return (bytes_before + 15) & ~(size_t)15; }
inline size_t prop_tab_offset(size_t P) { return prop_table_at(22 * P); }

__host__ __device__ __forceinline__ uint32_t prop_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float prop_uniform(uint32_t x)   // [-1, 1) in steps of 2^-23, every operation exact
{
    return ((float)(int32_t)(x >> 8) - 8388608.0f) * (1.0f / 8388608.0f);
}

__device__ __forceinline__ bool prop_inside(float z) { return z > -1.0f && z < 1.0f; }   // false for NaN

// rule 4: argmin_update_packed<CS_FIXED>'s comparison of two packed cells (the products stay below 2^32: s < 2^24, k < 2^8)
__device__ __forceinline__ bool prop_better(uint32_t c, uint32_t b)
{
    return (c >> 24) != 0u && (b == 0u || umul24u(c & 0xffffffu, b >> 24) < umul24u(b & 0xffffffu, c >> 24));
}

// the support byte of pixel `pix`: behind the cost map come the guide bytes, then the support bytes
__device__ __forceinline__ uint8_t *prop_support_at(const SweepParams &p, const PropArgs &a, size_t pix)
{
    int W = p.W, H = p.H;
    asm volatile("" : "+s"(W), "+s"(H));   // (computed where it is used, twice per pixel, not held in registers through the kernel)
    const size_t P = (size_t)W * H;
    return (uint8_t *)(a.cost + P) + P + pix;
}

// section 27, rules 2-6: the penalty g of the hypothesis depth cz at (row, col), in units of the cells' sums per counted view, and the
// number of listed neighbours that answer for it.  f32, one rounding per operation, in fusion's order (depth_rules.hpp).  `geo` is the
// table in LDS: every lane reads the same element, a broadcast.  No branches: a lane whose neighbour does not answer computes on a
// valid address and discards what it gets (its wave would wait for the others anyway), which keeps the execution masks of three nested
// tests out of the scalar registers.  The scheduling barriers keep the table's reads of one step from being issued ahead of the step
// before it, so at most one camera matrix (16 registers) is live at a time
__device__ __forceinline__ uint32_t prop_consistency(const SweepParams &p, const PropGeo *geo, int nslots, int row, int col, float cz, uint32_t &answers)
{
    // Nothing computed here may be taken for an invariant of the candidate loop and kept in registers through the window loops, where the
    // kernel needs the most: the table's address, the pixel and the frame's size pass through empty asm statements, which the compiler
    // cannot see through
    int opaque = 0, W = p.W, H = p.H;
    asm volatile("" : "+v"(opaque), "+v"(row), "+v"(col), "+s"(W), "+s"(H));
    const PropGeo &g = *(const PropGeo *)((const char *)geo + opaque);
    const float *M = g.cam[0];
    const float halfW = (float)W * 0.5f, halfH = (float)H * 0.5f;
    const float xn = __builtin_fmaf((float)(2 * col + 1), p.invW, -1.0f);
    const float yn = __builtin_fmaf(-(float)(2 * row + 1), p.invH, 1.0f);
    const float3 X = unproject(M + 16, xn, yn, cz);
    const float max_px = g.max_px, w255 = g.w255;
    uint32_t sum = 0u;
    answers = 0u;
#pragma unroll 1
    for (int j = 0; j < nslots; j++) {
        __builtin_amdgcn_sched_barrier(0);
        const float *Pj = g.cam[j + 1];
        const float qw = prow(Pj, 3, X);
        const float ax = prow(Pj, 0, X) / qw, ay = prow(Pj, 1, X) / qw;
        const float u = (ax + 1.0f) * halfW - 0.5f;
        const float v = (1.0f - ay) * halfH - 0.5f;
        const float fc = floorf(u + 0.5f), fr = floorf(v + 0.5f);
        const bool in = qw > 0.f && fc >= 0.f && fc < (float)W && fr >= 0.f && fr < (float)H;       // false for NaN
        const float zj = g.map[j][in ? (int)fr * W + (int)fc : 0];                                   // (the frame has fewer than 2^28 pixels)
        __builtin_amdgcn_sched_barrier(0);
        const float3 Xj = unproject(Pj + 16, ax, ay, zj);   // the continuous position with the nearest pixel's depth
        __builtin_amdgcn_sched_barrier(0);
        const float sw = prow(M, 3, Xj);
        const float ur = (prow(M, 0, Xj) / sw + 1.0f) * halfW - 0.5f;
        const float vr = (1.0f - prow(M, 1, Xj) / sw) * halfH - 0.5f;
        const float du = ur - (float)col, dv = vr - (float)row;
        const float d = sqrtf(du * du + dv * dv);
        const bool answer = in && prop_inside(zj) && sw > 0.f && d <= max_px;   // rule 5 (d NaN: no)
        answers += answer ? 1u : 0u;
        sum += (uint32_t)floorf((answer ? d : max_px) * w255);
    }
    return sum / (uint32_t)nslots;
}

template <int COST, int R, int KMAX>
__global__ __launch_bounds__(ZN_THREADS) void propagate_pass(SweepParams p, const uint32_t *__restrict__ lut_g, PropArgs a)
{
    using S = ZnShape<R>;
    using C = BkCost<COST>;
    using Elem = typename C::Elem;
    constexpr bool ZNCC = COST == MVS_COST_ZNCC;
    __shared__ uint32_t lut[1024];
    __shared__ uint8_t mainl[S::SAMPLES];   // [HH][HW] the main image of tile + halo (0 outside the frame: such a member is never sampled)
    __shared__ uint8_t guidel[S::SAMPLES];  // [HH][HW] the gate's guide likewise: the main image again, or the stage's copy of the caller's
    __shared__ PropGeo geol;                // section 27's table (filled only with a term)
    __shared__ PropCold coldl;              // the arguments of the random candidates and the counters' address
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ZN_TW, y0 = blockIdx.y * ZN_TH;
#pragma unroll
    for (int i = 0; i < 4; i++) lut[tid + ZN_THREADS * i] = lut_g[tid + ZN_THREADS * i];
    for (int i = tid; i < S::SAMPLES; i += ZN_THREADS) {
        const int hy = i / S::HW, hx = i - hy * S::HW;
        const int col = x0 - R + hx, row = y0 - R + hy;
        const bool in = col >= 0 && col < p.W && row >= 0 && row < p.H;
        const size_t at = in ? (size_t)row * p.W + col : 0;
        const uint8_t m = in ? p.main_img[at] : (uint8_t)0;
        mainl[i] = m;
        guidel[i] = (in && a.guide) ? a.guide[at] : m;
    }
    if (tid == 0) {
        coldl.dz = a.dz;
        coldl.dg = a.dg;
        coldl.seed = a.seed;
        coldl.counters = a.counters;
    }
    if (a.nslots)
        for (int i = tid; i < PROP_GEO_WORDS; i += ZN_THREADS) ((uint32_t *)&geol)[i] = ((const uint32_t *)a.geo)[i];
    __syncthreads();   // the only barrier: everything below is per thread
    const float hix = ZN_MAGIC + 132.0f + 256.0f * (float)p.W, hiy = ZN_MAGIC + 132.0f + 256.0f * (float)p.H;
    const bool init = a.half < 0;
    const int ly = tid / (ZN_TW / 2), j = tid - ly * (ZN_TW / 2);
    const int row = y0 + ly;
    int cls = -1;   // the class of what the pixel holds at the end of its list; -1: not an active pixel of the frame
    for (int s = 0; s < (init ? 2 : 1); s++) {
        const int lx = 2 * j + (init ? s : ((row + a.half) & 1));
        const int col = x0 + lx;
        if (col >= p.W || row >= p.H) continue;
        const size_t pix = (size_t)row * p.W + col;
        float z = a.z[pix], gx = a.gx[pix], gy = a.gy[pix];
        uint32_t cell = init ? 0u : a.cells[pix];
        cls = PR_KEPT;
        const uint32_t g0 = guidel[(ly + R) * S::HW + lx + R];
        const int ncand = init ? 1 : 8 + a.nrandom;
        for (int ci = 0; ci < ncand; ci++) {
            // the candidate (cz, cgx, cgy); cz = NaN: there is none (such a candidate has no counted view and never wins)
            float cz = __builtin_nanf(""), cgx = 0.0f, cgy = 0.0f;
            int ccls;
            if (init) {
                cz = z, cgx = gx, cgy = gy;
                ccls = PR_KEPT;
            } else if (ci < 8) {
                const int d = ci < 4 ? 1 : 5;
                const int dc = (ci & 2) ? 0 : ((ci & 1) ? d : -d), dr = (ci & 2) ? ((ci & 1) ? d : -d) : 0;   // (-d,0) (d,0) (0,-d) (0,d)
                const int nc = col + dc, nr = row + dr;
                ccls = ci < 4 ? PR_NEAR : PR_FAR;
                if (nc >= 0 && nc < p.W && nr >= 0 && nr < p.H) {
                    const size_t n = (size_t)nr * p.W + nc;
                    const float zn = a.z[n];
                    if (prop_inside(zn)) {
                        cgx = a.gx[n];
                        cgy = a.gy[n];
                        cz = (zn - cgx * (float)dc) - cgy * (float)dr;   // the neighbour's plane extended to this pixel
                    }
                }
            } else {
                ccls = PR_RANDOM;
                if (prop_inside(z)) {
                    int opaque = 0;
                    asm volatile("" : "+v"(opaque));   // (read here, per candidate, not once for the kernel and then held)
                    const PropCold &cold = *(const PropCold *)((const char *)&coldl + opaque);
                    const uint32_t base = prop_mix(cold.seed ^ (uint32_t)(row * p.W + col));
                    const uint32_t k = 4u * (uint32_t)(ci - 8);
                    cz = z + cold.dz * prop_uniform(prop_mix(base ^ k));
                    cgx = gx + cold.dg * prop_uniform(prop_mix(base ^ (k + 1u)));
                    cgy = gy + cold.dg * prop_uniform(prop_mix(base ^ (k + 2u)));
                }
            }
            if (!prop_inside(cz)) continue;   // the centre is not live: cell 0
            // rules 1-3: the candidate's cell
            BkList<KMAX> acc;
            acc.clear();
            for (int v = p.v0; v < p.v0 + p.vcount; v++) {
                const float *q = p.Q + 12 * v;
                const uint32_t *qv = p.quads + p.pad_slab * (size_t)(p.view_slot ? p.view_slot[v] : v);
                const float bx = q[2], by = q[6], bw = q[10];
                Elem sum;
                if constexpr (ZNCC)
                    sum = make_uint4(0u, 0u, 0u, 0u);
                else
                    sum = 0u;
                uint32_t centre_ok = 0u;
#pragma unroll 1
                for (int dr = -R; dr <= R; dr++) {
                    const int qr = row + dr;
                    const float yn = __builtin_fmaf(-(float)(2 * qr + 1), p.invH, 1.0f);
                    const float zr = cgy * (float)dr;
#pragma unroll 1
                    for (int dc = -R; dc <= R; dc++) {
                        const int qc = col + dc;
                        const bool in = (qc >= 0) & (qc < p.W) & (qr >= 0) & (qr < p.H);   // (no short circuit: one mask, no branch in the window loop)
                        const float zq = (cz + cgx * (float)dc) + zr;
                        const uint32_t gq = guidel[(ly + dr + R) * S::HW + lx + dc + R];
                        const bool gate = max(gq, g0) - min(gq, g0) <= (uint32_t)a.tau;
                        const float zs = (in && gate && prop_inside(zq)) ? zq : __builtin_nanf("");   // not live: the sampler's s.w > 0 test rejects NaN
                        const float xn = __builtin_fmaf((float)(2 * qc + 1), p.invW, -1.0f);
                        const Affine A = view_affine(q, xn, yn);
                        const uint32_t am = mainl[(ly + dr + R) * S::HW + lx + dc + R];
                        Elem e;
                        if constexpr (ZNCC)
                            e = zncc_sample(A, bx, by, bw, zs, qv, (uint32_t)p.pitch, hix, hiy, lut, am, am * am);
                        else
                            e = absdiff_sample(A, bx, by, bw, zs, qv, (uint32_t)p.pitch, hix, hiy, lut, 255u * am);
                        sum = C::add(sum, e);
                        if (dr == 0 && dc == 0) centre_ok = C::ok(e);
                    }
                }
                acc.insert(C::cost(sum, centre_ok));
            }
            uint32_t cc = acc.cell(a.keep);
            if (a.nslots && (init || (cc >> 24) != 0u)) {   // section 27, rule 7: k g on the sum (init: what it holds, counted or not, for the support map)
                uint32_t answers;
                const uint32_t g = prop_consistency(p, &geol, a.nslots, row, col, cz, answers), k = cc >> 24;
                cc = k ? cc + k * g : 0u;
                // rule 8: the count travels with the hypothesis.  A candidate that wins writes its own at once (the last winner's stays); a
                // pixel that keeps what it holds keeps its byte; init, whose one candidate is what the pixel holds, writes it win or not
                // (a pixel without a hypothesis never comes here: init's host side has cleared the map)
                if (init || prop_better(cc, cell)) prop_support_at(p, a, pix)[0] = (uint8_t)answers;
            }
            if (prop_better(cc, cell)) {
                z = cz, gx = cgx, gy = cgy;
                cell = cc;
                cls = ccls;
            }
        }
        a.z[pix] = z;
        a.gx[pix] = gx;
        a.gy[pix] = gy;
        a.cells[pix] = cell;
        a.cost[pix] = cell ? cell_cost<CS_FIXED>(cell & 0xffffffu, cell >> 24) : __builtin_inff();
    }
    if (!init) {
        // the report's counters: one ballot and one atomic per wave and class
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long m = __ballot(cls == k);
            if (m != 0ull && (tid & 63) == 0) atomicAdd(coldl.counters + k, (unsigned long long)__popcll(m));
        }
    }
}

// rule 5: the start map -> z (invalid values become the background depth) and the slopes.  `src` may be the z map itself: a pixel then
// rewrites its own value only, with the value it holds or, for an invalid one, with another invalid one, so what a neighbour reads of
// it means the same before and after
__global__ __launch_bounds__(256) void propagate_seed(const float *src, float *z, float *gx, float *gy, int W, int H, int slopes, float max_step)
{
    const int col = blockIdx.x * 32 + (threadIdx.x & 31), row = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (col >= W || row >= H) return;
    const size_t pix = (size_t)row * W + col;
    const float zp = src[pix];
    const bool has = prop_inside(zp);
    float g[2] = {0.0f, 0.0f};
    if (has && slopes) {
#pragma unroll
        for (int ax = 0; ax < 2; ax++) {
            const int at = ax ? row : col, n = ax ? H : W;
            const size_t stride = ax ? (size_t)W : 1;
            const float zm = at > 0 ? src[pix - stride] : __builtin_nanf(""), zq = at + 1 < n ? src[pix + stride] : __builtin_nanf("");
            const bool um = prop_inside(zm) && fabsf(zm - zp) <= max_step, uq = prop_inside(zq) && fabsf(zq - zp) <= max_step;
            g[ax] = um && uq ? (zq - zm) * 0.5f : uq ? zq - zp : um ? zp - zm : 0.0f;
        }
    }
    z[pix] = has ? zp : MVS_BACKGROUND_DEPTH;
    gx[pix] = g[0];
    gy[pix] = g[1];
}

// one launch of the pass kernel on the recorded cost, radius, keep and view range
void pass(mvs_ctx *ctx, PropArgs &a)
{
    const size_t P = (size_t)ctx->W * ctx->H;
    float *maps = (float *)ctx->prop_maps.ptr;
    a.z = maps;
    a.gx = maps + P;
    a.gy = maps + 2 * P;
    a.cells = (uint32_t *)(maps + 3 * P);
    a.cost = maps + 4 * P;
    a.counters = (unsigned long long *)ctx->prop_counters.ptr;
    a.keep = ctx->prop_keep;
    a.tau = ctx->prop_tau;
    a.guide = ctx->prop_guide_own ? (const uint8_t *)(maps + 5 * P) : nullptr;
    a.nslots = ctx->prop_geo_n;
    a.geo = (const PropGeo *)((const char *)maps + prop_tab_offset(P));
    SweepParams p;
    fill_params(ctx, p, ctx->prop_view_first, ctx->prop_view_count, ZN_TH, ZN_PC);
    const dim3 grid((unsigned)div_up(ctx->W, ZN_TW), (unsigned)div_up(ctx->H, ZN_TH));
    const uint32_t *lut = (const uint32_t *)ctx->fx_lut.ptr;
    with_bestk_shape<0>(ctx->prop_cost, ctx->prop_radius, a.keep, [&](auto c, auto r, auto kmax) {
        propagate_pass<decltype(c)::value, decltype(r)::value, decltype(kmax)::value><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, a);
    });
}

// what init and run refuse alike: the staged state the sampler reads
int staged_state(mvs_ctx *ctx, const char *who)
{
    if (!ctx->have_main || !ctx->have_views) return fail(ctx, MVS_ESTATE, "%s: set main view and side views first", who);
    if (ctx->sampler != MVS_SAMPLER_FIXED) return fail(ctx, MVS_ESTATE, "%s: implemented for MVS_SAMPLER_FIXED (the library default)", who);
    return MVS_OK;
}

// section 27, rule 7: the largest penalty a candidate can get, floorf(max_px * weight * 255) (the setter admits up to 1 000 000)
float consistency_cap(float weight, float max_px) { return floorf(max_px * (weight * 255.0f)); }

// what init refuses with a term recorded; `tab` gets the table of rule 1 (the main camera's matrices made as a slot's are, the
// neighbours' as their slots hold them, where their maps are), and nothing of the context changes
int consistency_stage(mvs_ctx *ctx, const char *who, int keep, int view_count, PropGeo &tab)
{
    const int n = ctx->prop_cons_n, cap = (int)ctx->dstore.size();
    if (cap == 0) return fail(ctx, MVS_ESTATE, "%s: a geometric term is recorded and there is no depth store (mvs_depth_store)", who);
    for (int j = 0; j < n; j++) {
        const int s = ctx->prop_cons_slots[j];
        if (s >= cap) return fail(ctx, MVS_ESTATE, "%s: neighbour slot %d of the geometric term is outside the depth store (capacity %d)", who, s, cap);
        if (!ctx->dstore[s].have) return fail(ctx, MVS_ESTATE, "%s: neighbour slot %d of the geometric term holds no depth map (mvs_depth_upload)", who, s);
    }
    mvs_ctx::DepthSlot m;
    if (!slot_matrices(ctx->main_cam, m)) return fail(ctx, MVS_EINVAL, "%s: a geometric term is recorded and the main camera is singular or has no finite centre", who);
    // the cells' 24-bit sums: k (65025 + g) must stay below 2^24 for every k the merge can give (rule 7 covers k <= 8)
    const int kmax = keep == MVS_KEEP_ALL ? view_count : keep;
    if ((double)kmax * (65025.0 + (double)consistency_cap(ctx->prop_cons_weight, ctx->prop_cons_max_px)) >= 16777216.0)
        return fail(ctx, MVS_EINVAL, "%s: %d views under MVS_KEEP_ALL with a geometric term of up to %g per view overflow the cells' 24-bit sums (set keep <= 8)", who,
                    view_count, (double)consistency_cap(ctx->prop_cons_weight, ctx->prop_cons_max_px));
    const size_t P = (size_t)ctx->W * ctx->H;
    memcpy(tab.cam[0], m.P, sizeof(m.P));
    memcpy(tab.cam[0] + 16, m.Pi, sizeof(m.Pi));
    for (int j = 0; j < n; j++) {
        const mvs_ctx::DepthSlot &s = ctx->dstore[ctx->prop_cons_slots[j]];
        memcpy(tab.cam[j + 1], s.P, sizeof(s.P));
        memcpy(tab.cam[j + 1] + 16, s.Pi, sizeof(s.Pi));
        tab.map[j] = (const float *)ctx->dstore_depth.ptr + P * ctx->prop_cons_slots[j];
    }
    tab.w255 = ctx->prop_cons_weight * 255.0f;
    tab.max_px = ctx->prop_cons_max_px;
    return MVS_OK;
}

// what run refuses with the term of the last init: the kernel reads the store's maps where they were then
int consistency_current(mvs_ctx *ctx, const char *who)
{
    bool moved = ctx->dstore.size() != ctx->prop_geo_cap;
    for (int j = 0; j < ctx->prop_geo_n && !moved; j++)   // (re-sized and back: the buffers grow only, but they may have moved)
        moved = ctx->prop_geo.map[j] != (const float *)ctx->dstore_depth.ptr + (size_t)ctx->W * ctx->H * ctx->prop_geo_slots[j];
    if (moved)
        return fail(ctx, MVS_ESTATE, "%s: the depth store was re-sized since mvs_propagate_init took its geometric term (capacity %d then, %d now)", who,
                    (int)ctx->prop_geo_cap, (int)ctx->dstore.size());
    for (int j = 0; j < ctx->prop_geo_n; j++)
        if (!ctx->dstore[ctx->prop_geo_slots[j]].have)
            return fail(ctx, MVS_ESTATE, "%s: neighbour slot %d of the geometric term holds no depth map any more", who, ctx->prop_geo_slots[j]);
    return MVS_OK;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_propagate_init(mvs_ctx *ctx, const void *depth_dev, int view_first, int view_count, int cost, int radius, int keep, float max_step, unsigned flags)
{
    static const char who[] = "mvs_propagate_init";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!depth_dev) return fail(ctx, MVS_EINVAL, "%s: depth_dev is null", who);
    int rc;
    if ((rc = bestk_arguments(ctx, who, cost, radius, keep))) return rc;
    if (flags & ~MVS_PROPAGATE_SLOPES) return fail(ctx, MVS_EINVAL, "%s: unknown flag bits 0x%x (MVS_PROPAGATE_SLOPES only)", who, flags & ~MVS_PROPAGATE_SLOPES);
    if (!(max_step >= 0.0f)) return fail(ctx, MVS_EINVAL, "%s: max_step %g is negative or NaN", who, (double)max_step);
    if ((flags & MVS_PROPAGATE_SLOPES) && ctx->dfit_seed_gx)
        return fail(ctx, MVS_EINVAL, "%s: MVS_PROPAGATE_SLOPES with recorded slopes (mvs_propagate_set_slopes): one source of slopes only", who);
    if ((rc = staged_state(ctx, who))) return rc;
    if ((rc = fx_sampler_limits(ctx, who, view_first, view_count))) return rc;
    PropGeo tab = {};
    if (ctx->prop_cons_n > 0 && (rc = consistency_stage(ctx, who, keep, view_count, tab))) return rc;
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    const size_t maps_bytes = 5 * P * sizeof(float) + P;   // z, gx, gy, the cells, the cost map; the gate's guide (u8)
    // behind them the support map (u8) and, on a 16-byte boundary, the geometric term's table
    if ((rc = ensure(ctx, ctx->prop_maps, prop_table_at(maps_bytes + P) + sizeof(PropGeo)))) return rc;
    if ((rc = ensure(ctx, ctx->prop_counters, 4 * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure_fx_lut(ctx))) return rc;
    ctx->prop_cost = cost;
    ctx->prop_radius = radius;
    ctx->prop_keep = keep;
    ctx->prop_view_first = view_first;
    ctx->prop_view_count = view_count;
    ctx->prop_iter = 0;
    ctx->prop_tau = ctx->prop_gate_tau;
    ctx->prop_guide_own = ctx->prop_gate_guide != nullptr;
    float *maps = (float *)ctx->prop_maps.ptr;
    if (ctx->prop_guide_own) MVS_HIP(ctx, hipMemcpyAsync(maps + 5 * P, ctx->prop_gate_guide, P, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->prop_geo_n = ctx->prop_cons_n;
    ctx->prop_geo_cap = ctx->dstore.size();
    if (ctx->prop_geo_n > 0) {
        memcpy(ctx->prop_geo_slots, ctx->prop_cons_slots, sizeof(ctx->prop_geo_slots));
        ctx->prop_geo = tab;   // the copy below reads the context's table, which lives as long as the stage
        MVS_HIP(ctx, hipMemcpyAsync((char *)maps + prop_tab_offset(P), &ctx->prop_geo, sizeof(PropGeo), hipMemcpyHostToDevice, ctx->stream));
    }
    MVS_HIP(ctx, hipMemsetAsync((uint8_t *)(maps + 5 * P) + P, 0, P, ctx->stream));   // rule 8: 0 without a term, and for a pixel without a hypothesis
    MVS_HIP(ctx, hipMemsetAsync(ctx->prop_counters.ptr, 0, 4 * sizeof(unsigned long long), ctx->stream));
    {
        ProfileScope ps(ctx, MVS_K_SWEEP);
        const dim3 grid((unsigned)div_up(ctx->W, 32), (unsigned)div_up(ctx->H, 8));
        propagate_seed<<<grid, 256, 0, ctx->stream>>>((const float *)depth_dev, maps, maps + P, maps + 2 * P, ctx->W, ctx->H, (flags & MVS_PROPAGATE_SLOPES) ? 1 : 0, max_step);
        dfit_seed_slopes(ctx, maps, maps + P, maps + 2 * P);   // section 32: the recorded slope seeds, consumed here
        PropArgs a = {};
        a.half = -1;
        pass(ctx, a);
    }
    MVS_HIP(ctx, hipGetLastError());
    ctx->prop_have = true;
    return MVS_OK;
}

int mvs_propagate_run(mvs_ctx *ctx, int iterations, float dz, float dg, int nrandom, unsigned seed)
{
    static const char who[] = "mvs_propagate_run";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (iterations < 1) return fail(ctx, MVS_EINVAL, "%s: iterations %d below 1", who, iterations);
    if (nrandom < 0 || nrandom > 4) return fail(ctx, MVS_EINVAL, "%s: nrandom %d outside 0..4", who, nrandom);
    if (!(dz >= 0.0f) || !std::isfinite(dz) || !(dg >= 0.0f) || !std::isfinite(dg))
        return fail(ctx, MVS_EINVAL, "%s: dz %g / dg %g negative or not finite", who, (double)dz, (double)dg);
    int rc;
    if ((rc = staged_state(ctx, who))) return rc;
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "%s: no hypotheses yet (mvs_propagate_init first)", who);
    if (ctx->prop_view_first + ctx->prop_view_count > ctx->V)
        return fail(ctx, MVS_ESTATE, "%s: the views changed since mvs_propagate_init: its range [%d,%d) is outside 0..%d", who, ctx->prop_view_first,
                    ctx->prop_view_first + ctx->prop_view_count, ctx->V);
    if (ctx->prop_geo_n > 0 && (rc = consistency_current(ctx, who))) return rc;
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_fx_lut(ctx))) return rc;
    {
        ProfileScope ps(ctx, MVS_K_SWEEP);
        for (int i = 0; i < iterations; i++) {
            const long long t = ctx->prop_iter + i;
            PropArgs a = {};
            a.dz = dz;
            a.dg = dg;
            for (long long k = 0; k < t && (a.dz != 0.0f || a.dg != 0.0f); k++) {   // halved t times, one rounding each
                a.dz *= 0.5f;
                a.dg *= 0.5f;
            }
            a.nrandom = nrandom;
            for (int h = 0; h < 2; h++) {
                a.half = h;
                a.seed = prop_mix(seed + (uint32_t)(2 * t + h));
                pass(ctx, a);
            }
        }
    }
    MVS_HIP(ctx, hipGetLastError());
    ctx->prop_iter += iterations;
    return MVS_OK;
}

int mvs_propagate_set_gate(mvs_ctx *ctx, int tau, const void *guide_dev)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_set_gate: null context");
    if (tau < 0 || tau > 255) return fail(ctx, MVS_EINVAL, "mvs_propagate_set_gate: tau %d outside 0..255", tau);
    ctx->prop_gate_tau = tau;
    ctx->prop_gate_guide = guide_dev;
    return MVS_OK;
}

int mvs_propagate_set_consistency(mvs_ctx *ctx, int nslots, const int *slots, float weight, float max_px)
{
    static const char who[] = "mvs_propagate_set_consistency";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (nslots < 0 || nslots > PROP_MAX_SLOTS) return fail(ctx, MVS_EINVAL, "%s: nslots %d outside 0..%d", who, nslots, PROP_MAX_SLOTS);
    if (nslots > 0) {
        if (!slots) return fail(ctx, MVS_EINVAL, "%s: slots is null", who);
        for (int j = 0; j < nslots; j++)
            if (slots[j] < 0) return fail(ctx, MVS_EINVAL, "%s: slot %d is negative", who, slots[j]);
        if (!(weight >= 0.0f) || !std::isfinite(weight)) return fail(ctx, MVS_EINVAL, "%s: weight %g negative or not finite", who, (double)weight);
        if (!(max_px > 0.0f) || !std::isfinite(max_px)) return fail(ctx, MVS_EINVAL, "%s: max_px %g not positive or not finite", who, (double)max_px);
        if (!(consistency_cap(weight, max_px) <= 1000000.0f))
            return fail(ctx, MVS_EINVAL, "%s: floor(max_px * weight * 255) = %g above 1000000: the cells' sums have 24 bits", who, (double)consistency_cap(weight, max_px));
    }
    ctx->prop_cons_n = nslots;
    for (int j = 0; j < PROP_MAX_SLOTS; j++) ctx->prop_cons_slots[j] = j < nslots ? slots[j] : 0;
    ctx->prop_cons_weight = nslots > 0 ? weight : 0.0f;
    ctx->prop_cons_max_px = nslots > 0 ? max_px : 0.0f;
    return MVS_OK;
}

void *mvs_propagate_support_device(mvs_ctx *ctx) { return ctx && ctx->prop_have ? (uint8_t *)((float *)ctx->prop_maps.ptr + 5 * (size_t)ctx->W * ctx->H) + (size_t)ctx->W * ctx->H : nullptr; }

int mvs_propagate_support_fetch(mvs_ctx *ctx, uint8_t *support_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_support_fetch: null context");
    if (!support_hw) return fail(ctx, MVS_EINVAL, "mvs_propagate_support_fetch: support_hw is null");
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "mvs_propagate_support_fetch: no hypotheses yet (mvs_propagate_init first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(support_hw, mvs_propagate_support_device(ctx), (size_t)ctx->W * ctx->H, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_propagate_fetch(mvs_ctx *ctx, float *z_hw, float *gx_hw, float *gy_hw, uint32_t *cells_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_fetch: null context");
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "mvs_propagate_fetch: no hypotheses yet (mvs_propagate_init first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    const float *maps = (const float *)ctx->prop_maps.ptr;
    void *const out[4] = {z_hw, gx_hw, gy_hw, cells_hw};
    for (int i = 0; i < 4; i++)
        if (out[i]) MVS_HIP(ctx, hipMemcpyAsync(out[i], maps + i * P, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

void *mvs_propagate_depth_device(mvs_ctx *ctx) { return ctx && ctx->prop_have ? ctx->prop_maps.ptr : nullptr; }

void *mvs_propagate_cost_device(mvs_ctx *ctx) { return ctx && ctx->prop_have ? (float *)ctx->prop_maps.ptr + 4 * (size_t)ctx->W * ctx->H : nullptr; }

int mvs_propagate_report(mvs_ctx *ctx, long long out[5])
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_report: null context");
    if (!out) return fail(ctx, MVS_EINVAL, "mvs_propagate_report: out is null");
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "mvs_propagate_report: no hypotheses yet (mvs_propagate_init first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    std::vector<uint32_t> cells(P);
    unsigned long long counters[4];
    MVS_HIP(ctx, hipMemcpyAsync(counters, ctx->prop_counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipMemcpyAsync(cells.data(), (const float *)ctx->prop_maps.ptr + 3 * P, P * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++) out[k] = (long long)counters[k];
    out[4] = 0;
    for (size_t i = 0; i < P; i++) out[4] += cells[i] != 0u;
    return MVS_OK;
}
