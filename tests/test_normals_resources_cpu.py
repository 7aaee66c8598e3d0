"""Resources of the normals' kernels (csrc/normals.hip) from the compiler's report for gfx950 with the Makefile's own
CXXFLAGS: no scratch, no spills; registers, occupancy and LDS are printed (section 31's table is this output).  The four fusion kernels of
csrc/fuse.hip keep the registers they had (sections 11 and 28): rules 3n and 5n leave no trace in them.  And by source inspection: the two
new buffers are allocated only by the calls the section names, behind their last refusal, and named nowhere else."""
import os
import re

from kernel_resources import PKG, fixture

KEYS = ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")
NEW = ("hypothesis_normals_kernel", "fuse_count_normals_kernel", "fuse_rows_normals_kernel")
BEFORE = {"fuse_count_kernel": 26, "fuse_rows_kernel": 30, "fuse_count_masked_kernel": 26, "fuse_rows_masked_kernel": 30}   # VGPRs, sections 11 and 28


resources = fixture("normals.hip", "fuse.hip")


def _ours(resources, kernel):
    names = [n for n in resources if re.search(r"\d%sE" % kernel, n) and "rocprim" not in n]
    assert len(names) == 1, (kernel, sorted(n for n in resources if "rocprim" not in n))
    return resources[names[0]]


def test_no_scratch_no_spills_and_the_fusion_kernels_keep_their_registers(resources):
    ours = [n for n in resources if "rocprim" not in n]
    assert len(ours) == len(NEW) + len(BEFORE), sorted(ours)
    for kernel in NEW + tuple(BEFORE):
        k = _ours(resources, kernel)
        row = tuple(int(k[key]) for key in KEYS)
        print("%-26s %3d VGPRs, %3d SGPRs, %d waves/SIMD, %4d bytes LDS" % ((kernel,) + row[:4]))
        assert row[4:] == (0, 0, 0), (kernel, k)
    for kernel, vgprs in BEFORE.items():
        assert int(_ours(resources, kernel)["VGPRs"]) == vgprs, (kernel, _ours(resources, kernel))
    # the normals cost the two new fusion kernels a few registers: the same eight waves per SIMD and the same tile in LDS
    for kernel in NEW[1:]:
        assert int(_ours(resources, kernel)["Occupancy [waves/SIMD]"]) == int(_ours(resources, "fuse_rows_kernel")["Occupancy [waves/SIMD]"])
        assert int(_ours(resources, kernel)["LDS Size [bytes/block]"]) == int(_ours(resources, "fuse_rows_kernel")["LDS Size [bytes/block]"])
    assert int(_ours(resources, NEW[0])["LDS Size [bytes/block]"]) == 0


def _sources():
    out = {}
    for name in os.listdir(os.path.join(PKG, "csrc")):
        out[name] = open(os.path.join(PKG, "csrc", name), errors="replace").read()
    return out


def _body(text, start, end="\n}\n"):
    return text[text.index(start):text.index(end, text.index(start))]


def test_the_buffers_are_allocated_only_by_the_named_calls_behind_the_last_refusal():
    src = _sources()
    assert sorted(n for n, t in src.items() if "store_normals" in t) == ["context.hip", "fuse.hip", "mvs_internal.hpp", "normals.hip"]
    assert sorted(n for n, t in src.items() if "hyp_normals" in t) == ["context.hip", "mvs_internal.hpp", "normals.hip"]
    assert "&ctx->store_normals, &ctx->hyp_normals," in src["context.hip"] and src["context.hip"].count("store_normals") == 1 == src["context.hip"].count("hyp_normals")   # the list mvs_destroy frees
    text = src["normals.hip"]
    assert "hipMalloc" not in text and sum(t.count("ensure(ctx, ctx->store_normals") + t.count("ensure(ctx, ctx->hyp_normals") for t in src.values()) == 2
    # the planes: both uploads go through one function, which allocates behind its last refusal and sets the flag behind the copy
    upload = _body(text, "int normals_upload_impl(")
    assert text.count("normals_upload_impl(") == 3
    assert upload.count("ensure(ctx, ctx->store_normals") == 1 and upload.index("ensure(ctx, ctx->store_normals") > upload.rindex("return fail(")
    assert upload.index("have_normals = true") > upload.index("hipMemcpyAsync")
    # mvs_depth_store frees them, a depth upload only clears the slot's flag, the drop too
    store = _body(src["fuse.hip"], "int mvs_depth_store(")
    assert "hipFree(ctx->store_normals.ptr)" in store and "ensure(ctx, ctx->store_normals" not in store
    depth_upload = _body(src["fuse.hip"], "int depth_upload_impl(")
    assert "have_normals = false" in depth_upload and "store_normals" not in depth_upload
    assert "have_normals = false" in _body(text, "int mvs_depth_normals_drop(") and "store_normals" not in _body(text, "int mvs_depth_normals_drop(")
    # the fusion takes a plane's address only for a slot that has one
    fuse = _body(text, "int mvs_fuse_depth_normals(")
    lines = [line for line in fuse.splitlines() if "store_normals.ptr" in line]
    assert len(lines) == 1 and "have_normals ?" in lines[0] and ": nullptr" in lines[0], lines
    assert "ensure(ctx, ctx->store_normals" not in fuse and "ensure(ctx, ctx->hyp_normals" not in fuse
    first = fuse.index("ensure(ctx, ")
    assert max(m.start() for m in re.finditer(r"return fail\(ctx, MVS_E(INVAL|STATE)", fuse)) < first and fuse.index("fuse_check_slots(") < first
    assert fuse.index("fuse_fill_args(") < fuse.index("<<<")
    assert len(re.findall(r"hipStreamSynchronize", fuse)) == 2 and fuse.index("if (out_points7 && total > 0) {") < fuse.rindex("hipStreamSynchronize")
    # the map of mvs_propagate_normals: made by that call alone, behind every check; the call does not wait
    call = _body(text, "int mvs_propagate_normals(")
    assert call.count("ensure(ctx, ctx->hyp_normals") == 1 and call.index("ensure(ctx, ctx->hyp_normals") > call.rindex("return fail(")
    assert call.index("hyp_normals_have = true") > call.index("<<<") and "Synchronize" not in call and "hipMemcpy" not in call
    assert "prop_maps" not in text and "dstore_support" not in text
