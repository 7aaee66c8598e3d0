"""Resources of the propagation's kernels with the geometric term in them (csrc/propagate.hip) from the compiler's
report for gfx950 with the Makefile's own CXXFLAGS: the same 36 instantiations of propagate_pass and propagate_seed -- the term is runtime
arguments --, none with scratch or spills; registers, occupancy and LDS are printed (section 27's table is this output).  And by source
inspection: mvs_propagate_set_consistency allocates nothing, the stage still has its two ensure calls behind init's last refusal, and the
term's checks sit in front of them."""
import os


from kernel_resources import PKG
from test_propagate_resources_cpu import INSTANCES, resources  # noqa: F401  (the fixture: one compilation of the file per module)

KEYS = ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")


def test_the_36_instantiations(resources):
    assert len(resources) == 37, sorted(resources)
    rows = []
    for cost, r, kmax in INSTANCES:
        names = [n for n in resources if "14propagate_passILi%dELi%dELi%dEE" % (cost, r, kmax) in n]
        assert len(names) == 1, (cost, r, kmax)
        k = resources[names[0]]
        rows.append((("absdiff", "zncc")[cost], r, kmax) + tuple(int(k[key]) for key in KEYS))
        print("%-7s r = %d KMAX = %d: %3d VGPRs, %3d SGPRs, %d waves/SIMD, %4d bytes LDS" % rows[-1][:7])
    assert all(row[7:] == (0, 0, 0) for row in rows), [row for row in rows if row[7:] != (0, 0, 0)]
    # the term's table (1232 bytes) and the cold arguments (24) are static LDS of every instantiation, beside the weights and the two tiles:
    # far from the 160 KiB of a compute unit that would cap eight workgroups
    assert all(row[6] <= 8192 for row in rows), max(row[6] for row in rows)


def _source():
    return open(os.path.join(PKG, "csrc", "propagate.hip")).read()


def test_the_setter_allocates_nothing():
    src = _source()
    body = src[src.index("int mvs_propagate_set_consistency("):src.index("void *mvs_propagate_support_device(")]
    for word in ("ensure(", "hipMalloc", "hipMemcpy", "hipMemset", "hipSetDevice", "<<<", "prop_maps", "prop_geo"):
        assert word not in body, word
    assert body.count("return fail(") == 7 and body.index("ctx->prop_cons_n = nslots") > body.rindex("return fail("), "nothing is recorded by a refused call"


def test_the_stage_still_has_its_two_allocations_behind_every_check():
    src = _source()
    assert src.count("hipMalloc") == 0 and src.count("ensure(ctx, ctx->prop_") == 2
    init = src[src.index("int mvs_propagate_init("):src.index("int mvs_propagate_run(")]
    assert init.count("ensure(ctx, ctx->prop_") == 2
    assert init.index("consistency_stage(") < init.index("ensure(ctx, ctx->prop_maps") and init.rindex("return fail(") < init.index("ensure(ctx, ctx->prop_maps")
    assert init.index("ctx->prop_geo_n = ") > init.index("ensure(ctx, ctx->prop_counters"), "what init takes is recorded behind the allocations"
    run = src[src.index("int mvs_propagate_run("):src.index("int mvs_propagate_set_gate(")]
    assert run.index("consistency_current(") < run.index("hipSetDevice") and "ensure(ctx, ctx->prop_" not in run
    # the support map and the table live in the one allocation: no new buffer of the context
    hpp = open(os.path.join(PKG, "csrc", "mvs_internal.hpp")).read()
    assert hpp.count("mvs::DevBuf prop_") == 1 and "prop_maps, prop_counters;" in hpp
    assert open(os.path.join(PKG, "csrc", "context.hip")).read().count("prop_") == 2
