"""The CPU oracle and the argument handling of the C ABI against RECORDED RESULTS OF THE REFERENCE ITSELF
(tests/golden/reference_sweep.json, written by tests/golden/make_reference_sweep.py from the reference as
oracle/build_ref.py compiles it under the mock AviSynth host).  Needs no device.

The fixture alone suffices for the oracle tests.  Where oracle/_ref/libref_mock_avs.so exists the fixture is also
regenerated in memory (the staleness check) and the reference's error strings are compared with the C ABI's; those
tests skip only where the binary is absent."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_reference_sweep", os.path.join(ROOT, "tests", "golden", "make_reference_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load_generator()
ROWS = M.load()["cases"]
RECORDED = ("out_dims", "crc32", "crc32_frame", "chroma_location")
NO_BINARY = "oracle/_ref/libref_mock_avs.so is absent (oracle/build_ref.py builds it where the reference's sources are available)"


@pytest.fixture(scope="module")
def ref():
    L = M.reference_library()
    if L is None:
        pytest.skip(NO_BINARY)
    return L


def oracle_frame(O, row, src=None):
    """The oracle's frame for a fixture row: float arguments are the recorded float32 values, as doubles."""
    fmt = O.FORMATS[row["format"]]
    for k, bits in row["args_f32_bits"].items():    # the decimal beside the bit pattern is that float32 value exactly
        assert M.f32_bits(row["args"][k]) == int(bits, 16) and M.f32(row["args"][k]) == row["args"][k]
    from conftest import oracle_kwargs
    of = O.OracleFilter(fmt, *row["src"], *row["dst"], **oracle_kwargs(M.oracle_args(row)))
    return of, (src if src is not None else M.source_frame(O, row))


def first_difference(O, L, row, got_planes, what):
    """Where the binary is present: the first sample at which `got_planes` leaves the reference's frame."""
    if L is None:
        return f"{what}: crc differs from the recorded reference result (no reference binary here to localise it)"
    planes, (w, h), _ = M.run_host(L, O, row)
    for i, (pw, ph) in enumerate(O.FORMATS[row["format"]].plane_dims(w, h)):
        a, b = np.ascontiguousarray(got_planes[i][:ph, :pw]), np.ascontiguousarray(planes[i][:ph, :pw])
        if a.dtype == np.float32:
            nan = np.isnan(a) & np.isnan(b)
            a, b = np.where(nan, 0, a.view(np.uint32)), np.where(nan, 0, b.view(np.uint32))
        bad = np.argwhere(a != b)
        if len(bad):
            y, x = bad[0]
            return (f"{what}: plane {i} differs from the reference at {len(bad)} samples; first (x={x}, y={y}): "
                    f"got {got_planes[i][y, x]!r}, reference {planes[i][y, x]!r}")
    return f"{what}: crc differs from the fixture but the frame equals the reference's of this build: the fixture is stale"


def test_fixture_rows_are_the_generators_cases():
    """Every case of the generator is on file with the parameters it has today (no device, no binary needed)."""
    cases = M.cases()
    assert [r["name"] for r in ROWS] == [c["name"] for c in cases]
    for r, c in zip(ROWS, cases):
        assert {k: v for k, v in r.items() if k not in RECORDED} == c, r["name"]
        assert all(k in r for k in RECORDED)
    assert 85 <= len(ROWS) <= 110
    small = [r for r in ROWS if not r.get("gpu_only") and not r["opt"]]
    assert all(r["out_dims"][0] <= 400 and r["out_dims"][1] <= 260 for r in small)
    assert sum(1 for r in ROWS if r["opt"]) == 18 and {r["opt"] for r in ROWS} == {0, 1, 2, 3}


def test_small_cases_are_those_of_the_parity_suite():
    import test_gpu_parity
    want = [c for c in test_gpu_parity.SMALL_CASES if c[3] <= 400 and c[4] <= 260]
    assert M.SMALL_CASES == want


def test_sweep_covers_the_argument_surface(O):
    sweep = [r for r in ROWS if r["name"].startswith("sweep")]
    fmts = {r["format"] for r in ROWS if not r["opt"]}
    assert {O.FORMATS[f].bits for f in fmts} == {8, 10, 12, 14, 16, 32}
    assert {(O.FORMATS[f].planes, O.FORMATS[f].sub_w, O.FORMATS[f].sub_h, O.FORMATS[f].rgb) for f in fmts} >= {
        (1, 0, 0, False), (3, 1, 1, False), (3, 1, 0, False), (3, 2, 0, False), (3, 0, 0, False), (3, 0, 0, True), (4, 0, 0, True),
        (4, 1, 1, False), (4, 1, 0, False), (4, 0, 0, False)}
    assert len({r["format"] for r in sweep}) >= 16
    assert {M.oracle_args(r).get("tap", 3) for r in ROWS} >= set(range(1, 17))
    assert {r["function"] for r in sweep} == {"JincResize", *M.ALIAS_TAPS}
    assert {r["args"]["cplace"].lower() for r in ROWS if "cplace" in r["args"]} == {"mpeg2", "mpeg1", "topleft"}
    ratios = [r["dst"][0] / r["src"][0] for r in sweep] + [r["dst"][1] / r["src"][1] for r in sweep]
    assert min(ratios) < 0.5 and max(ratios) > 3.0
    assert any(r["args"].get("src_left", 0) < 0 for r in sweep) and any(r["args"].get("src_width", 1) <= 0 for r in sweep)
    quants = [r["args"][k] for r in sweep for k in ("quant_x", "quant_y") if k in r["args"]]
    assert min(quants) <= 8 and max(quants) >= 200
    blurs = [r["args"]["blur"] for r in sweep if "blur" in r["args"]]
    assert 0.8 <= min(blurs) < 0.9 and 1.25 < max(blurs) <= 1.3


@pytest.mark.parametrize("name,crc", sorted(M.VERDICT_SCRIPT_FLOATS.items()))
def test_fixture_holds_the_verdicts_script_float_answers(name, crc):
    """The seven answers of VERDICT r6 (an independent run of the reference) are what this build of the reference recorded:
    the recipe of oracle/build_ref.py is cross-checked by them."""
    row = next(r for r in ROWS if r["name"] == name)
    assert row["crc32_frame"] == crc


@pytest.mark.parametrize("name", sorted(n for n in M.VERDICT_SCRIPT_FLOATS if "C4" not in n))
def test_own_build_of_the_reference_reproduces_the_verdicts_small_answers(ref, O, name):
    row = next(r for r in ROWS if r["name"] == name)
    planes, (w, h), _ = M.run_host(ref, O, row)
    assert M.frame_crc(planes, O.FORMATS[row["format"]].plane_dims(w, h)) == M.VERDICT_SCRIPT_FLOATS[name]


@pytest.mark.parametrize("row", [r for r in ROWS if not r["opt"] and not r.get("gpu_only")], ids=lambda r: r["name"])
def test_oracle_reproduces_the_reference_opt0(O, row):
    """oracle/jinc_oracle.c + the derivation in oracle/oracle.py, fed the float32-rounded arguments, against the reference's
    own frame: crc per plane, output size, and the _ChromaLocation the reference wrote (2 for every sub-sampled format)."""
    of, src = oracle_frame(O, row)
    out = of.get_frame(src, threads=4)
    assert [of.target_w, of.target_h] == row["out_dims"]
    got = M.plane_crcs(out, of.out_dims())
    if got != row["crc32"]:
        pytest.fail(first_difference(O, M.reference_library(), row, out, f"oracle, {row['name']}, plane crcs {got} vs {row['crc32']}"))
    fmt = O.FORMATS[row["format"]]
    assert row["chroma_location"] == (2 if (fmt.sub_w or fmt.sub_h) else None)


@pytest.mark.parametrize("row", [r for r in ROWS if r["opt"]], ids=lambda r: r["name"])
def test_oracle_simd_orders_reproduce_the_reference_opt123(O, row):
    """oracle/simd_order.c (every opt), simd_avx2.c (opt=2) and simd_avx512.c (opt=3, where the CPU has it) against the
    reference's SSE4.1 / AVX2 / AVX-512 frames."""
    of, src = oracle_frame(O, row)
    order = row["opt"]
    out = of.get_frame_simd(order, src, threads=4)
    got = M.plane_crcs(out, of.out_dims())
    if got != row["crc32"]:
        pytest.fail(first_difference(O, M.reference_library(), row, out, f"simd_order.c order {order}, {row['name']}"))
    if order == 2 and O.lib().oracle_avx2_available():
        out = of.get_frame_simd(2, src, threads=4, avx2=True)
        assert M.plane_crcs(out, of.out_dims()) == row["crc32"], first_difference(O, M.reference_library(), row, out, "simd_avx2.c")
    if order == 3:
        if not O.lib().oracle_avx512_available():
            pytest.skip("simd_order.c order 3 checked; simd_avx512.c needs AVX-512, which this CPU lacks")
        out = of.get_frame_simd(3, src, threads=4, avx512=True)
        assert M.plane_crcs(out, of.out_dims()) == row["crc32"], first_difference(O, M.reference_library(), row, out, "simd_avx512.c")


def test_simd_non_finite_rows_hold_what_they_are_for(O):
    """Two rows per opt put NaN, -inf and denormals -- and no +inf, whose answer in the reference depends on memory to the right of
    the window -- into every source plane; the recorded chroma crcs are not the luma clamp's: NaN and -inf become the plane's
    min_val (0 on plane 0, -0.5 on planes 1 and 2), which simd_order.c reproduces above only with the right one."""
    rows = [r for r in ROWS if r["opt"] and "nonfinite_seed" in r]
    assert sorted((r["opt"], r["format"]) for r in rows) == [(o, f) for o in (1, 2, 3) for f in ("Y32", "YUV444PS")]
    for row in rows:
        assert row["nonfinite_kinds"] == list(M.NO_POS_INF)
        of, src = oracle_frame(O, row)
        assert {1: 7, 3: 9}[len(src)] == of.tables[0].filter_size   # tap 3 (an unrolled size of the kernel) and tap 4 at 1.5x
        for p, (w, h) in zip(src, O.FORMATS[row["format"]].plane_dims(*row["src"])):
            v = p[:h, :w]
            assert not np.isposinf(v).any() and np.isneginf(v).any() and np.isnan(v).any()
            assert ((np.abs(v) < np.float32(1.1754944e-38)) & (v != 0)).any()
        if len(src) == 3:   # the clamp by plane kind is visible in these rows: chroma under the luma clamp gives another plane
            wrong = O.alloc_plane(*of.out_dims()[1], np.float32)
            of.tables[0].resize_simd(row["opt"], src[1], wrong, 0.0, threads=4)
            assert M.plane_crc(wrong, *of.out_dims()[1]) != row["crc32"][1]


def test_simd_rows_differ_from_opt0_where_the_orders_do(O):
    """The C1-shaped rows are the 3 / 7 / 7 differing pixels of SURVEY 0: the opt rows pin something opt=0 does not."""
    c1 = {r["opt"]: r for r in ROWS if "C1_640x360" in r["name"]}
    of, src = oracle_frame(O, c1[1])
    want0 = of.get_frame(src, threads=4)[0][:720, :1280]
    for order, n in ((1, 3), (2, 7), (3, 7)):
        out = of.get_frame_simd(order, src, threads=4)[0][:720, :1280]
        assert int((out != want0).sum()) == n
        assert M.plane_crc(out, 1280, 720) == c1[order]["crc32"][0]


def test_fixture_is_what_the_reference_binary_gives_today(ref, O):
    """The staleness check: regenerating the fixture in memory from oracle/_ref/libref_mock_avs.so gives the committed file,
    entry for entry (the one full-size row excepted: it is recorded once and checked on the GPU only)."""
    new = M.generate(include_gpu_only=False, previous=ROWS)
    assert len(new) == len(ROWS)
    for a, b in zip(new, ROWS):
        if a != b:
            of, src = oracle_frame(O, b)
            out = of.get_frame_simd(b["opt"], src, threads=4) if b["opt"] else of.get_frame(src, threads=4)
            pytest.fail(f"{b['name']}: regenerated {({k: a[k] for k in RECORDED})} != committed {({k: b[k] for k in RECORDED})}; "
                        + first_difference(O, ref, b, out, "oracle"))


# ------------------------------------------------------------------------------------------------------------------
# error behaviour: the reference's returned string against jinc_filter_create's, call by call
# ------------------------------------------------------------------------------------------------------------------
ALL_FLAGS = M.CPUF_SSE41 | M.CPUF_AVX2 | M.CPUF_AVX512F
# (format, named script arguments, host: cpu_flags / planar / frame-0 _ChromaLocation)
BAD_CALLS = [
    ("Y8", dict(tap=0), {}), ("Y8", dict(tap=17), {}), ("YUV420P8", dict(tap=-1), {}), ("RGBPS", dict(tap=100), {}),
    ("Y8", dict(quant_x=0), {}), ("Y8", dict(quant_x=257), {}), ("YUV444P16", dict(quant_x=-8), {}),
    ("Y8", dict(quant_y=0), {}), ("Y8", dict(quant_y=257), {}), ("Y16", dict(quant_y=1000), {}),
    ("Y8", dict(cplace="jpeg"), {}), ("YUV420P8", dict(cplace="left"), {}), ("YUV420P8", dict(cplace="top left"), {}),
    ("Y8", dict(cplace="topleft"), {}), ("YUV422P8", dict(cplace="TopLeft"), {}), ("YUV411P8", dict(cplace="topleft"), {}),
    ("YUV444P8", dict(cplace="TOPLEFT"), {}), ("RGBP8", dict(cplace="topleft"), {}), ("YUVA422P10", dict(cplace="topleft"), {}),
    ("Y8", dict(opt=4), {}), ("Y8", dict(opt=100), {}),
    ("Y8", dict(opt=3), dict(cpu_flags=M.CPUF_SSE41 | M.CPUF_AVX2)), ("Y8", dict(opt=2), dict(cpu_flags=M.CPUF_SSE41)),
    ("Y8", dict(opt=1), dict(cpu_flags=0)), ("Y16", dict(opt=3), dict(cpu_flags=0)),
    ("Y8", dict(threads=2), {}), ("Y8", dict(threads=-1), {}),
    ("Y8", dict(initial_factor=0.5), {}), ("Y8", dict(initial_factor=0.99), {}),
    ("Y8", dict(initial_capacity=0), {}), ("Y8", dict(initial_capacity=-3), {}),
    ("Y8", {}, dict(planar=0)), ("YUV420P8", dict(tap=99), dict(planar=0)),
    ("YUV420P8", {}, dict(chroma_location=4)), ("YUV420P8", {}, dict(chroma_location=3)), ("YUV420P8", {}, dict(chroma_location=255)),
    ("YUV422P8", {}, dict(chroma_location=2)),
    # validation order (ref :700-789): tap, quant_x, quant_y, cplace, topleft, opt, threads, initial_factor, initial_capacity
    ("Y8", dict(tap=99, quant_x=999, cplace="bogus"), {}), ("Y8", dict(quant_x=999, quant_y=999, cplace="bogus"), {}),
    ("Y8", dict(quant_y=999, cplace="bogus", opt=9), {}), ("Y8", dict(cplace="bogus", opt=9, threads=5), {}),
    ("YUV422P8", dict(cplace="topleft", opt=9), {}), ("Y8", dict(opt=9, threads=5), {}),
    ("Y8", dict(threads=5, initial_factor=0.1), {}), ("Y8", dict(initial_factor=0.1, initial_capacity=0), {}),
]


def _reference_error(L, O, fmt_name, named, tw=128, th=96, cpu_flags=ALL_FLAGS, planar=1, chroma_location=-1):
    env = M.Env(L, cpu_flags)
    src = env.source(O.FORMATS[fmt_name], 64, 48, None, planar=planar, chroma_location=chroma_location)
    clip, err = env.invoke("JincResize", src, tw, th, named)
    if clip:
        L.mock_clip_release(clip)
    L.mock_source_release(src)
    env.close()
    return err


def _abi_error(pkg, fmt_name, named, tw=128, th=96, cpu_flags=ALL_FLAGS, planar=1, chroma_location=-1, with_code=False):
    try:
        pkg.Filter(pkg.FORMATS[fmt_name], 64, 48, tw, th, device=-1, planar=bool(planar), frame0_chroma_location=chroma_location,
                   cpu_flags=(bool(cpu_flags & M.CPUF_SSE41), bool(cpu_flags & M.CPUF_AVX2), bool(cpu_flags & M.CPUF_AVX512F)),
                   **named).close()
    except pkg.JincError as e:
        return f"{e} (code {e.code})" if with_code else str(e)
    return None


def test_bad_call_list_is_long_enough():
    assert len(BAD_CALLS) >= 25


@pytest.mark.parametrize("fmt_name,named,host", BAD_CALLS,
                         ids=[f"{f}_" + "_".join(f"{k}{v}" for k, v in {**n, **h}.items()).replace(" ", "") for f, n, h in BAD_CALLS])
def test_error_string_is_the_references(ref, O, pkg, fmt_name, named, host):
    """The reference's own returned error against the string jinc_filter_create produces without a device."""
    want = _reference_error(ref, O, fmt_name, named, **host)
    assert want is not None and want.startswith("JincResize: ")
    assert _abi_error(pkg, fmt_name, named, **host, with_code=True) == want + " (code -1)"   # -1: the reference's own refusals


def test_good_calls_are_good_on_both_sides(ref, O, pkg):
    """The neighbours of the bad calls: accepted by the reference and by the C ABI alike."""
    for fmt_name, named, host in (("Y8", dict(tap=1), {}), ("Y8", dict(tap=16, quant_x=1, quant_y=256), {}), ("YUV420P8", dict(cplace="TOPLEFT"), {}),
                                  ("YUV420P8", dict(cplace=""), {}), ("Y8", dict(opt=3, threads=1), {}), ("Y8", dict(opt=-1), dict(cpu_flags=0)),
                                  ("Y8", dict(blur=0.0, initial_factor=1.0, initial_capacity=1), {}), ("YUV420P8", {}, dict(chroma_location=2)),
                                  ("YUV422P8", {}, dict(chroma_location=1))):
        assert _reference_error(ref, O, fmt_name, named, **host) is None, (fmt_name, named, host)
        assert _abi_error(pkg, fmt_name, named, **host) is None, (fmt_name, named, host)


def test_degenerate_sizes_are_refused_where_the_reference_is_not(ref, O, pkg):
    """Not "the same error string": calls the reference ACCEPTS and this project refuses on purpose (csrc/plan.h: geometry the
    reference handles only through out-of-bounds reads or degenerate sizes).  A target of zero width or height gives the
    reference a filter with an empty output; a relative crop that leaves no source gives it a negative crop width.  Recorded
    here from the reference itself so that the deviation stays a stated one."""
    for tw, th in ((0, 96), (128, 0)):
        assert _reference_error(ref, O, "Y8", {}, tw=tw, th=th) is None
        assert _abi_error(pkg, "Y8", {}, tw=tw, th=th) == "JincResize: plane dimensions must be positive."
    assert _reference_error(ref, O, "Y8", dict(src_width=-70.0)) is None
    assert _abi_error(pkg, "Y8", dict(src_width=-70.0)) == "JincResize: source crop must have positive width and height."
