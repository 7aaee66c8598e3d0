// fuse_sequence.hip -- sequence fusion (include/mvs.h "sequence fusion"): mvs_fuse_sequence runs the per-pixel
// contract of mvs_fuse_depth_masked (csrc/fuse_rules.hpp, the same statements) for a list of reference slots in list order and emits every
// surface point once: a kept pixel marks, in a claim plane per slot, the pixel of every neighbour that agreed with it, and a marked pixel
// starts no point of its own when its slot's turn as the reference comes.
//
// Per reference four launches on the context's stream, none of which the host waits for:
//   fuse_seq_count_kernel    keep count per segment, as fuse_count_kernel, with `claim_ref[p] == 0` in the keep test; writes no claims (the
//                            row pass runs the same pixels);
//   rocprim exclusive scan   segment offsets within the reference (32-bit: one reference has at most H*W rows);
//   fuse_seq_rows_kernel     recomputes the pixels, writes the rows at (running total + offset) where that index is below max_rows (64-bit:
//                            8191 slots at 1080p exceed 2^31 rows), and stores 1 at rule 3's pixel of every neighbour that agreed;
//   fuse_seq_advance_kernel  one thread: per-reference count out, running total += count.
// The launches of reference i read claim plane ref_i only and write planes of other slots only (a neighbour equal to its reference is
// refused), every store writes the value 1, and the launches are stream-ordered: the result does not depend on scheduling.  The call
// synchronises once for the total and the per-reference counts, and once more when rows are downloaded.
//
// tests/fuse_sequence_mirror.py restates the contract in numpy, bit for bit.
#include "fuse_rules.hpp"
#include "mvs_internal.hpp"

#include <rocprim/rocprim.hpp>

#include <cmath>
#include <vector>

namespace mvs {

namespace {

struct FuseSeqArgs : FuseMaskedArgs {
    const uint8_t *claim_ref;                 // the reference slot's claim plane (read only)
    uint8_t *claim[kFuseMaxNeighbours + 1];   // [j]: neighbour j's claim plane (written only); [0] unused
};

// WRITE = false: keep count per segment and counts[H * ntx] = 0; WRITE = true: rows behind *base at the scanned offsets, and the claims
template <bool WRITE>
__device__ __forceinline__ void fuse_seq_body(const FuseSeqArgs &a, int *__restrict__ counts, const int *__restrict__ offsets, const long long *__restrict__ base,
                                              long long max_rows, float *__restrict__ rows)
{
    __shared__ float4 tile[kFuseTY + 2][kFuseTX + 2];
    const int tx = threadIdx.x & (kFuseTX - 1), ty = threadIdx.x / kFuseTX;
    const int col0 = blockIdx.x * kFuseTX, row0 = blockIdx.y * kFuseTY;
    fuse_load_tile(a, tile, row0, col0);
    const int row = row0 + ty, col = col0 + tx;
    float out[7];
    unsigned agreed = 0u;
    // S2: a claimed pixel starts no point; it is still in the tile above (a tangent neighbour) and still votes in other references' rule 3
    const bool keep = row < a.H && col < a.W && a.claim_ref[(size_t)row * a.W + col] == 0 && fuse_pixel(a, tile, ty + 1, tx + 1, row, col, out, agreed);
    const unsigned long long m = __ballot(keep);
    const int seg = row * a.ntx + blockIdx.x;
    if (!WRITE) {
        if (tx == 0 && row < a.H) counts[seg] = __popcll(m);
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) counts[a.H * a.ntx] = 0;
    } else if (keep) {
        const long long at = *base + (long long)(offsets[seg] + __popcll(m & ((1ull << tx) - 1ull)));
        if (at < max_rows) {  // S4: a row that does not fit is not written; its claims are made all the same
            float *dst = rows + 7 * (size_t)at;
            for (int k = 0; k < 7; k++) dst[k] = out[k];
        }
        // S3: the pixel rule 3 read in every neighbour that agreed (the same statements as the vote's: vote_pixel)
        const float4 c = tile[ty + 1][tx + 1];
        const float3 X = make_float3(c.x, c.y, c.z);
        for (int j = 1; j <= a.K; j++) {
            if (!(agreed >> (j - 1) & 1u)) continue;
            int rj, cj;
            if (vote_pixel(a, j, X, rj, cj)) a.claim[j][(size_t)rj * a.W + cj] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void fuse_seq_count_kernel(const FuseSeqArgs a, int *__restrict__ counts)
{
    fuse_seq_body<false>(a, counts, nullptr, nullptr, 0, nullptr);
}

__global__ __launch_bounds__(256) void fuse_seq_rows_kernel(const FuseSeqArgs a, const int *__restrict__ offsets, const long long *__restrict__ base,
                                                            long long max_rows, float *__restrict__ rows)
{
    fuse_seq_body<true>(a, nullptr, offsets, base, max_rows, rows);
}

// behind a reference's row pass: its count out, the running total moved on (one thread)
__global__ void fuse_seq_advance_kernel(const int *__restrict__ count, long long *__restrict__ total, int *__restrict__ ref_count)
{
    *ref_count = *count;
    *total = *total + (long long)*count;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_fuse_sequence(mvs_ctx *ctx, int nrefs, const int *ref_slots, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px,
                      float max_rel_depth, float max_cost, int min_support, long long max_rows, float *out_points7, int *out_ref_counts, long long *out_count)
{
    const char *who = "mvs_fuse_sequence";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!out_count) return fail(ctx, MVS_EINVAL, "%s: out_count is null", who);
    *out_count = 0;
    const int cap = (int)ctx->dstore.size();
    if (nrefs < 1 || nrefs > cap) return fail(ctx, MVS_EINVAL, "%s: nrefs %d out of range 1..%d (the depth store's capacity)", who, nrefs, cap);
    if (!ref_slots) return fail(ctx, MVS_EINVAL, "%s: ref_slots is null", who);
    int rc;
    if ((rc = fuse_check_thresholds(ctx, who, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost, min_support))) return rc;
    if (max_rows < 0) return fail(ctx, MVS_EINVAL, "%s: max_rows %lld is negative", who, max_rows);
    // per reference the neighbours that are there (-1 = none), checked as mvs_fuse_depth_masked checks them; plane[slot] = the slot's claim plane
    std::vector<int> plane((size_t)cap, -1), lists((size_t)nrefs * (kFuseMaxNeighbours + 1));
    int nplanes = 0;
    for (int i = 0; i < nrefs; i++) {
        int *list = &lists[(size_t)i * (kFuseMaxNeighbours + 1)], n = 0;
        for (int j = 0; j < nneighbours; j++)
            if (neighbour_slots[(size_t)i * nneighbours + j] != -1) list[1 + n++] = neighbour_slots[(size_t)i * nneighbours + j];
        list[0] = n;
        if ((rc = fuse_check_slots(ctx, who, ref_slots[i], n, list + 1, max_cost, min_support))) return rc;
        for (int k = 0; k < i; k++)
            if (ref_slots[k] == ref_slots[i]) return fail(ctx, MVS_EINVAL, "%s: reference slot %d is listed twice (entries %d and %d)", who, ref_slots[i], k, i);
        for (int j = -1; j < n; j++) {
            const int slot = j < 0 ? ref_slots[i] : list[1 + j];
            if (plane[slot] < 0) plane[slot] = nplanes++;
        }
    }
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H;
    const size_t P = (size_t)W * H;
    const int ntx = div_up(W, kFuseTX);
    const size_t nseg = (size_t)H * ntx;
    const long long most = (long long)nrefs * (long long)P;
    const long long rows_cap = max_rows < most ? max_rows : most;  // rows the buffer holds: no index at or above it is written
    size_t scan_bytes = 0;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, (int *)nullptr, (int *)nullptr, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
        return fail(ctx, MVS_EHIP, "%s: scan sizing failed", who);
    ctx->fuse_seq_have_rows = false;
    if (rows_cap > 0 && (rc = ensure(ctx, ctx->fuse_seq_rows, (size_t)rows_cap * 7 * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->fuse_seq_claims, (size_t)nplanes * P))) return rc;
    if ((rc = ensure(ctx, ctx->fuse_seq_state, sizeof(long long) + (size_t)nrefs * sizeof(int)))) return rc;
    if ((rc = ensure(ctx, ctx->fuse_counts, 2 * (nseg + 1) * sizeof(int)))) return rc;
    if ((rc = ensure(ctx, ctx->fuse_scan, scan_bytes > 0 ? scan_bytes : 1))) return rc;
    int *counts = (int *)ctx->fuse_counts.ptr, *offsets = counts + nseg + 1;
    uint8_t *claims = (uint8_t *)ctx->fuse_seq_claims.ptr;
    long long *total = (long long *)ctx->fuse_seq_state.ptr;
    int *ref_counts = (int *)(total + 1);
    const size_t state_bytes = sizeof(long long) + (size_t)nrefs * sizeof(int);
    std::vector<char> state(state_bytes);
    const dim3 grid((unsigned)ntx, (unsigned)div_up(H, kFuseTY));
    {
        ProfileScope ps(ctx, MVS_K_FUSE);
        MVS_HIP(ctx, hipMemsetAsync(claims, 0, (size_t)nplanes * P, ctx->stream));  // S1
        MVS_HIP(ctx, hipMemsetAsync(total, 0, state_bytes, ctx->stream));
        for (int i = 0; i < nrefs; i++) {
            const int *list = &lists[(size_t)i * (kFuseMaxNeighbours + 1)];
            FuseSeqArgs a;
            memset((void *)&a, 0, sizeof(a));
            fuse_fill_args(ctx, a, ref_slots[i], list[0], list + 1, min_consistent, max_reproj_px, max_rel_depth, max_cost, min_support);
            a.claim_ref = claims + P * plane[ref_slots[i]];
            for (int j = 1; j <= list[0]; j++) a.claim[j] = claims + P * plane[list[j]];
            fuse_seq_count_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, counts);
            MVS_HIP(ctx, hipGetLastError());
            if (rocprim::exclusive_scan(ctx->fuse_scan.ptr, scan_bytes, counts, offsets, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
                return fail(ctx, MVS_EHIP, "%s: scan failed", who);
            fuse_seq_rows_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, offsets, total, rows_cap, (float *)ctx->fuse_seq_rows.ptr);
            MVS_HIP(ctx, hipGetLastError());
            fuse_seq_advance_kernel<<<1, 1, 0, ctx->stream>>>(offsets + nseg, total, ref_counts + i);
            MVS_HIP(ctx, hipGetLastError());
        }
    }
    MVS_HIP(ctx, hipMemcpyAsync(state.data(), total, state_bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    long long n = 0;
    memcpy(&n, state.data(), sizeof(n));
    if (out_ref_counts) memcpy(out_ref_counts, state.data() + sizeof(long long), (size_t)nrefs * sizeof(int));
    const long long fit = n < rows_cap ? n : rows_cap;
    if (out_points7 && fit > 0) {
        MVS_HIP(ctx, hipMemcpyAsync(out_points7, ctx->fuse_seq_rows.ptr, (size_t)fit * 7 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->fuse_seq_have_rows = true;
    *out_count = n;
    return MVS_OK;
}

void *mvs_fuse_sequence_points_device(mvs_ctx *ctx)
{
    if (!ctx) {
        fail(nullptr, MVS_EINVAL, "mvs_fuse_sequence_points_device: null context");
        return nullptr;
    }
    return ctx->fuse_seq_have_rows ? ctx->fuse_seq_rows.ptr : nullptr;
}

}  // extern "C"
