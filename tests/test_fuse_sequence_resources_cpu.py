"""Resources of the fusion kernels with the support planes and the sequence fusion in them (csrc/fuse.hip, csrc/fuse_sequence.hip, DESIGN.md
section 28) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no kernel of ours with scratch or spills, and
fuse_count_kernel / fuse_rows_kernel at the registers they had before (section 11).  Registers, occupancy and LDS are printed (section 28's
table is this output).  And by source inspection: the support buffer is allocated only by the support uploads, the sequence buffers only in
mvs_fuse_sequence behind its last refusal, and that call synchronises the stream exactly once when no rows are downloaded."""
import os
import re


from kernel_resources import PKG, fixture

KEYS = ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")
FUSE = ("fuse_count_kernel", "fuse_rows_kernel", "fuse_count_masked_kernel", "fuse_rows_masked_kernel")
SEQUENCE = ("fuse_seq_count_kernel", "fuse_seq_rows_kernel", "fuse_seq_advance_kernel")
BEFORE = {"fuse_count_kernel": 26, "fuse_rows_kernel": 30}   # VGPRs, DESIGN.md section 11


resources = fixture("fuse.hip", "fuse_sequence.hip")


def _ours(resources, kernel):
    names = [n for n in resources if re.search(r"\d%sE" % kernel, n) and "rocprim" not in n]
    assert len(names) == 1, (kernel, sorted(n for n in resources if "rocprim" not in n))
    return resources[names[0]]


def test_no_scratch_no_spills_and_the_old_kernels_keep_their_registers(resources):
    for kernel in FUSE + SEQUENCE:
        k = _ours(resources, kernel)
        row = tuple(int(k[key]) for key in KEYS)
        print("%-26s %3d VGPRs, %3d SGPRs, %d waves/SIMD, %4d bytes LDS" % ((kernel,) + row[:4]))
        assert row[4:] == (0, 0, 0), (kernel, k)
    for kernel, vgprs in BEFORE.items():
        assert int(_ours(resources, kernel)["VGPRs"]) == vgprs, (kernel, _ours(resources, kernel))
    # rule 1s and the claims cost the new kernels a few registers at most: the same eight waves per SIMD as the kernels they extend
    assert all(int(_ours(resources, k)["Occupancy [waves/SIMD]"]) == int(_ours(resources, "fuse_rows_kernel")["Occupancy [waves/SIMD]"]) for k in FUSE + SEQUENCE[:2])


def _sources():
    out = {}
    for name in os.listdir(os.path.join(PKG, "csrc")):
        out[name] = open(os.path.join(PKG, "csrc", name), errors="replace").read()
    return out


def _body(text, start, end):
    return text[text.index(start):text.index(end, text.index(start))]


def test_the_support_buffer_is_allocated_only_by_the_support_uploads():
    src = _sources()
    users = sorted(n for n, t in src.items() if "dstore_support" in t)
    assert users == ["context.hip", "fuse.hip", "mvs_internal.hpp", "tsdf.hip"], users
    assert src["context.hip"].count("dstore_support") == 1 and "&ctx->dstore_support," in src["context.hip"]   # the list mvs_destroy frees
    assert sum(t.count("ensure(ctx, ctx->dstore_support") for t in src.values()) == 1 and all("hipMalloc" not in src[n] for n in ("fuse.hip", "fuse_sequence.hip", "tsdf.hip"))
    upload = _body(src["fuse.hip"], "int support_upload_impl(", "\n}\n")
    assert upload.count("ensure(ctx, ctx->dstore_support") == 1 and upload.index("ensure(ctx, ctx->dstore_support") > upload.rindex("return fail(")
    assert upload.index("have_support = true") > upload.index("hipMemcpyAsync")
    # both uploads go through it; nothing else does
    assert src["fuse.hip"].count("support_upload_impl(") == 3
    # mvs_depth_store frees the buffer, a depth upload only clears the slot's flag
    store = _body(src["fuse.hip"], "int mvs_depth_store(", "\n}\n")
    assert "hipFree(ctx->dstore_support.ptr)" in store and "ensure(ctx, ctx->dstore_support" not in store
    depth_upload = _body(src["fuse.hip"], "int depth_upload_impl(", "\n}\n")
    assert depth_upload.count("have_support = false") == 2 and "dstore_support" not in depth_upload
    # the readers take the planes' address only under min_support > 0
    for name in ("fuse.hip", "tsdf.hip"):
        for line in src[name].splitlines():
            if "dstore_support.ptr +" in line and "support_upload_impl" not in line and "hipMemcpyAsync" not in line:
                assert "min_support > 0" in line, line


def test_the_sequence_buffers_are_allocated_only_in_mvs_fuse_sequence_behind_its_last_refusal():
    src = _sources()
    users = sorted(n for n, t in src.items() if "fuse_seq_rows" in t or "fuse_seq_claims" in t or "fuse_seq_state" in t)
    assert users == ["context.hip", "fuse_sequence.hip", "mvs_internal.hpp"], users
    assert "&ctx->fuse_seq_rows, &ctx->fuse_seq_claims, &ctx->fuse_seq_state," in src["context.hip"] and src["context.hip"].count("fuse_seq_") == 3
    text = src["fuse_sequence.hip"]
    call = _body(text, "int mvs_fuse_sequence(", "\nvoid *mvs_fuse_sequence_points_device(")
    assert text.count("ensure(ctx, ctx->fuse_seq_") == 3 == call.count("ensure(ctx, ctx->fuse_seq_")
    first = call.index("ensure(ctx, ")
    refusals = [m.start() for m in re.finditer(r"return fail\(ctx, MVS_E(INVAL|STATE)", call)]
    assert refusals and max(refusals) < first and call.index("fuse_check_slots(") < first and call.index("scan sizing failed") < first
    assert call.index("<<<") > call.rindex("ensure(ctx, ") and call.index("hipMemsetAsync") > call.rindex("ensure(ctx, ")


def test_one_synchronisation_without_a_download():
    text = _sources()["fuse_sequence.hip"]
    call = _body(text, "int mvs_fuse_sequence(", "\nvoid *mvs_fuse_sequence_points_device(")
    syncs = [m.start() for m in re.finditer(r"hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy\(|hipEventSynchronize", call)]
    assert len(syncs) == 2
    download = call.index("if (out_points7 && fit > 0) {")
    assert syncs[0] < download < syncs[1] < call.index("}", download), "the second one belongs to the optional row download"
    loop = _body(call, "for (int i = 0; i < nrefs; i++) {\n            const int *list", "MVS_HIP(ctx, hipMemcpyAsync(state.data()")
    assert "Synchronize" not in loop and loop.count("<<<") == 3 and "hipMemcpy" not in loop, "the host does not wait between references"
    # only the row pass writes claims
    body = _body(text, "__device__ __forceinline__ void fuse_seq_body(", "\n}\n")
    assert body.count("a.claim[j][") == 1 and body.index("a.claim[j][") > body.index("} else if (keep) {")
