"""The HIP kernels, through the C ABI and through the AviSynth shell under the mock host, against RECORDED RESULTS OF THE
REFERENCE ITSELF: tests/golden/reference_sweep.json (see tests/golden/make_reference_sweep.py for what a row holds and how
it was taken).  No oracle on this path: a row's crc32 per plane is the reference's, and an error that oracle and product
shared would show here.

The fixture alone suffices; oracle/_ref/libref_mock_avs.so, where present, only localises a mismatch.  Float planes follow
the suite's NaN rule (same NaN footprint, same bits elsewhere): every NaN counts as 0x7FC00000 in the crc."""
import numpy as np
import pytest

from test_plugin_mock_host import host  # noqa: F401  (session fixture: plugin + mock host in one library)
from test_reference_sweep_host import M, ROWS

pytestmark = pytest.mark.gpu

OPT0 = [r for r in ROWS if not r["opt"] and not r.get("gpu_only")]
GROUP = 8
GROUPS = [OPT0[i:i + GROUP] for i in range(0, len(OPT0), GROUP)]
GROUP_IDS = [f"{g[0]['name']}..{g[-1]['name']}" for g in GROUPS]

# (kernel mode, kernel that must then compute the interior of table 0) for each kernel-family row of the fixture, by the names of
# jinc_filter_last_kernel.  Mode 0 is the automatic choice at the row's shape.  The forms the automatic choice keeps for large
# calls (the two-period quad form, the runs form of the direct kernel; csrc/dispatch.cpp Rules) and the alternatives it has at
# these shapes are selected through jinc_filter_set_kernel_mode, so that they too are held to the reference's frame at a shape
# of a few milliseconds.  A dispatch change that takes a family off its row fails
# test_every_kernel_family_is_pinned_to_the_reference instead of silently dropping the family from the pin.
FAMILY_KERNELS = {
    "2x_tap3_u8": [(0, "ewa_periodic_kernel"), (13, "ewa_periodic_quad2_kernel")],
    "2x_tap4_u16": [(0, "ewa_periodic_quad8_kernel")],
    "2x_tap6_rowpair": [(0, "ewa_periodic_rowpair_kernel")],
    "2x_tap8_rowpair_420p16": [(0, "ewa_periodic_rowpair_kernel")],
    "3x": [(0, "ewa_gather_kernel"), (7, "ewa_quasi_kernel")],
    "4x": [(0, "ewa_periodic_kernel")],
    "1.37x_tap8": [(0, "ewa_gather_kernel")],
    "1.5x_tap8": [(0, "ewa_gather_kernel"), (14, "ewa_direct_runs_kernel")],
    "half_direct": [(0, "ewa_direct_kernel")],
    "five_sixths_direct": [(0, "ewa_gather_kernel")],     # (not exactly periodic at this size: the direct kernel is the half-scale row's)
    "tap12": [(0, "ewa_direct_kernel")],
    "drift_tap4_runs": [(14, "ewa_direct_runs_kernel")],
    "2x_tap4_float_quad": [(0, "ewa_periodic_quad9_kernel")],
}

REACHED = {}   # row name -> ([last_kernel of every table], last_instance of table 0), filled by abi_frame


def abi_frame(pkg, O, row, simd_order=0):
    """The row through the C ABI on device 0: float arguments are the recorded float32 values, handed over as doubles."""
    fmt = pkg.FORMATS[row["format"]]
    f = pkg.Filter(fmt, *row["src"], *row["dst"], device=0, **M.oracle_args(row))
    try:
        if simd_order:
            f.set_simd_order(simd_order)
        got = f.get_frame(M.source_frame(O, row))
        dims = f.out_dims()
        REACHED[row["name"]] = ([f.last_kernel(t) for t in range(f.num_tables)], f.last_instance(0))
        return got, dims, [f.dst_w, f.dst_h], f.chroma_location
    finally:
        f.close()


def explain(O, row, got, what):
    from test_reference_sweep_host import first_difference
    return first_difference(O, M.reference_library(), row, got, what)


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_c_abi_gives_the_references_frames(gpu_pkg, O, group):
    for row in group:
        got, dims, out_dims, loc = abi_frame(gpu_pkg, O, row)
        assert out_dims == row["out_dims"], row["name"]
        crcs = M.plane_crcs(got, dims)
        if crcs != row["crc32"]:
            pytest.fail(explain(O, row, got, f"C ABI, {row['name']} ({REACHED[row['name']]}), plane crcs {crcs} vs {row['crc32']}"))
        assert loc == (-1 if row["chroma_location"] is None else row["chroma_location"]), row["name"]


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_plugin_under_the_mock_host_gives_the_references_frames(host, gpu_pkg, O, monkeypatch, group):  # noqa: F811
    """The same script call the reference answered -- function (aliases included), named arguments, floats as 32-bit values,
    a host that reports no SIMD -- through plugin/jincresize_avs.cpp: frame, size and the _ChromaLocation property."""
    for var in ("JINCRESIZE_SIMD_ORDER", "JINCRESIZE_LOOKAHEAD", "JINCRESIZE_CHROMALOC", "JINCRESIZE_PIN_FRAMES", "JINCRESIZE_GROUP"):
        monkeypatch.delenv(var, raising=False)
    L = M.bind(host)
    for row in group:
        got, (w, h), loc = M.run_host(L, O, row)
        assert [w, h] == row["out_dims"], row["name"]
        crcs = M.plane_crcs(got, O.FORMATS[row["format"]].plane_dims(w, h))
        if crcs != row["crc32"]:
            pytest.fail(explain(O, row, got, f"plugin, {row['name']}, plane crcs {crcs} vs {row['crc32']}"))
        assert loc == row["chroma_location"], row["name"]


@pytest.mark.parametrize("opt", [1, 2, 3])
def test_simd_orders_give_the_references_opt_frames(gpu_pkg, O, opt):
    """jinc_filter_set_simd_order(1 / 2 / 3) against the reference's SSE4.1 / AVX2 / AVX-512 frames (8-bit at C1's shape, 16-bit,
    float, float 4:2:0, and the two float rows whose frames carry NaN, -inf and denormals: the lower clamp turns NaN and -inf
    into the plane's min_val, 0 on luma and -0.5 on chroma)."""
    rows = [r for r in ROWS if r["opt"] == opt]
    assert len(rows) == 6
    for row in rows:
        got, dims, out_dims, _ = abi_frame(gpu_pkg, O, row, simd_order=opt)
        assert set(REACHED[row["name"]][0]) == {"ewa_simd_order_kernel"}, REACHED[row["name"]]
        assert out_dims == row["out_dims"]
        crcs = M.plane_crcs(got, dims)
        if crcs != row["crc32"]:
            pytest.fail(explain(O, row, got, f"simd order {opt}, {row['name']}, plane crcs {crcs} vs {row['crc32']}"))


def test_non_finite_rows_hold_what_they_are_for(O):
    """The two non-finite rows really put +inf, -inf, NaN and denormals into every source plane (0 x inf -> NaN on the trimmed
    support is what they fix against the reference); they run with the other rows above."""
    rows = [r for r in OPT0 if "nonfinite_seed" in r]
    assert len(rows) == 2 and {M.oracle_args(r)["tap"] for r in rows} == {3, 4}
    for row in rows:
        assert row["dst"] == [2 * row["src"][0], 2 * row["src"][1]]
        for p, (w, h) in zip(M.source_frame(O, row), O.FORMATS[row["format"]].plane_dims(*row["src"])):
            v = p[:h, :w]
            assert np.isposinf(v).any() and np.isneginf(v).any() and np.isnan(v).any()
            assert ((np.abs(v) < np.float32(1.1754944e-38)) & (v != 0)).any()


def test_full_size_c4_with_the_scripts_blur(gpu_pkg, O):
    """C4 (RGBPS 3840 x 2160 -> 7680 x 4320, tap 4) with blur = (double)(float)0.98, what a script's blur=0.98 is: the
    reference's acd6b554 (575ed9a6 in tests/golden/kat.json answers the double 0.98, which only an ABI caller can pass)."""
    row = next(r for r in ROWS if r.get("gpu_only"))
    assert row["args"]["blur"] == float(np.float32(0.98)) and row["crc32_frame"] == "acd6b554"
    got, dims, out_dims, _ = abi_frame(gpu_pkg, O, row)
    assert out_dims == row["out_dims"]
    assert M.frame_crc(got, dims) == row["crc32_frame"]
    assert M.plane_crcs(got, dims) == row["crc32"]


def test_every_kernel_family_is_pinned_to_the_reference(gpu_pkg, O):
    """Each kernel family the dispatch can pick computes the interior of its fixture row -- by itself or selected through the
    test header's kernel mode -- and gives the reference's frame there."""
    rows = {r["family"]: r for r in OPT0 if "family" in r}
    assert set(rows) == set(FAMILY_KERNELS)
    reached = {}
    for label, row in rows.items():
        fmt = gpu_pkg.FORMATS[row["format"]]
        f = gpu_pkg.Filter(fmt, *row["src"], *row["dst"], device=0, **M.oracle_args(row))
        src = M.source_frame(O, row)
        for mode, _ in FAMILY_KERNELS[label]:
            f.set_kernel_mode(mode)
            got = f.get_frame(src)
            reached[label, mode] = f.last_kernel(0), f.last_instance(0)
            crcs = M.plane_crcs(got, f.out_dims())
            if crcs != row["crc32"]:
                pytest.fail(explain(O, row, got, f"{row['name']} kernel mode {mode} ({reached[label, mode]})"))
        f.close()
    print(reached)
    wrong = {k: (v[0], dict(FAMILY_KERNELS[k[0]])[k[1]]) for k, v in reached.items() if v[0] != dict(FAMILY_KERNELS[k[0]])[k[1]]}
    assert not wrong, f"(row, kernel mode): (kernel reached, kernel expected) {wrong}"
    assert {v[0] for v in reached.values()} >= {"ewa_periodic_kernel", "ewa_periodic_quad2_kernel", "ewa_periodic_quad8_kernel",
                                                "ewa_periodic_quad9_kernel", "ewa_periodic_rowpair_kernel",
                                                "ewa_gather_kernel", "ewa_quasi_kernel", "ewa_direct_kernel", "ewa_direct_runs_kernel"}
