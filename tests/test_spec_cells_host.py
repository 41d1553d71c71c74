"""The reference, the restated planners and the corpus of tests/spec_cells.py, checked without a
GPU: the corpus against the launch tables of spec.hip read as text, the planners' constants
against the sources, the launches every case must produce, the long-double reference against
scipy.signal, and every case's input conditions and e64."""

import os
import re

import numpy as np
import pytest

import spec_cells as C

CSRC = os.path.join(C.ROOT, "openseize_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_longdouble_is_80_bit():
    import scipy.fft
    C.assert_80_bit()
    assert scipy.fft.rfft(np.ones(12, C.LD)).dtype == np.complex256


def test_long_double_rfft_is_a_dft():
    """scipy.fft.rfft of a long-double array against the DFT summed directly in long double, at a
    prime, an odd composite and an odd length near 4096: within 4e-18 of the spectrum's rms."""
    import scipy.fft
    rng = np.random.default_rng(5)
    for n in (347, 1001, 4095):
        x = rng.standard_normal(n).astype(C.LD)
        k = np.arange(n // 2 + 1)
        ang = (np.outer(k, np.arange(n)) % n).astype(C.LD) * (2 * np.arccos(C.LD(-1)) / n)
        direct = (np.cos(ang) @ x) - 1j * (np.sin(ang) @ x)
        got = scipy.fft.rfft(x)
        err = float(np.abs(got - direct).max() / np.sqrt((np.abs(direct) ** 2).mean()))
        print(n, err)
        assert err < 4e-18 * np.sqrt(n)


def test_corpus_covers_the_launch_tables():
    """CASES and UNREACHED together are the full product of the launch tables; every instance has
    a ragged and a runs case, every mixed-radix and split instance a runs case with the
    half-carry and one without; the staged route runs in all modes and both detrends."""
    compiled = C.compiled_instances()
    assert len(compiled) == 12 + 60 + 30 + 18 + 30
    unreached = {u[0] for u in C.UNREACHED}
    for kind in ("ragged", "runs"):
        got = {c.want for c in C.CASES if c.kind == kind and c.want[0] != "staged"}
        assert got | unreached == compiled and not got & unreached, (kind, sorted(got ^ compiled)[:8])
    for inst in compiled:
        if inst[0] in ("mix", "split"):
            flags = {c.halfcarry for c in C.CASES if c.kind == "runs" and c.want == inst}
            assert flags == {0, 1}, (inst, flags)
    staged = {(c.mode, c.linear) for c in C.CASES if c.want[0] == "staged" and c.nfft == 4099 and c.nwin == 4099}
    assert staged == {(m, l) for m in C.MODES for l in (0, 1)}
    text = _src("spec.hip")
    for _, why, line in C.UNREACHED:
        assert why and text.count(line) == 1, line


def test_corpus_keeps_its_extras():
    """Beyond the instance cases: per family zero padding with an odd nwin, nwin = 2 and nwin = 1;
    every first-pass and every later-pass radix of the mixed-radix kernel; a prime, an even and
    an odd R0 of the split kernel with the workgroup sizes they take; R >= 2 on a head launch;
    the staged route under the three switches; and the cases of SUBSET_TAGS are those above
    LD_POINTS."""
    extra = [c for c in C.CASES if c.kind == "extra"]
    for fam in ("fft8", "mix", "split", "blue", "staged"):
        mine = [c for c in extra if c.want[0] == fam]
        assert any(2 < c.nwin < c.nfft and c.nwin % 2 == 1 for c in mine), fam
        assert any(c.nwin == 2 and c.nfft > 2 for c in mine), fam
        assert any(c.nwin == 1 and c.zero and not c.linear for c in mine), fam
        assert {c.mode for c in mine if c.nwin == 1} == set(C.MODES) == {c.mode for c in mine if c.nwin == 2}
    assert all(not c.zero or c.nwin == 1 for c in C.CASES)
    plans = [C.route(c.nwin, c.nfft, c.stride, dict(c.env)) for c in C.CASES]
    first = {r.radix[0] for r in plans if r.family == "mix"}
    later = {q for r in plans if r.family == "mix" for q in r.radix[1:]}
    alone = {r.radix[0] for r in plans if r.family == "mix" and len(r.radix) == 1}
    assert first == later == alone == {10, 4, 2, 3, 5, 7}
    r0 = {r.R0 for r in plans if r.family == "split"}
    assert {3, 5, 7, 11} <= r0 and 4 in r0                       # primes (odd: a self-paired workgroup), even
    assert {r.size for r in plans if r.family == "split" and r.R0 % 2} == {256, 512, 1024}
    later_split = {q for r in plans if r.family == "split" for q in r.radix[1:]}
    assert later_split == {10, 4, 2, 3, 5, 7}
    for fam in ("fft8", "mix", "blue"):
        heads = [r for c in extra if c.want[0] == fam for _, rs in C.plan_pushes(c) for r in rs if r["head"] == 1]
        assert any(r["R"] >= 2 and r["nruns"] >= 2 for r in heads), fam
    assert any(c.want[0] == "staged" and c.nfft == 4096 and len(c.env) == 3 for c in extra)
    assert any(c.want[0] == "blue" and c.nfft == 2 for c in extra) and any(c.nfft == 3 for c in extra)
    assert {C.tag(c) for c in C.CASES if C.uses_subset(c)} == set(C.SUBSET_TAGS)
    assert all(c.name in C.E64 for c in C.CASES) and len(C.E64) == len(C.CASES)


def test_a_new_instantiation_is_noticed():
    """A sixth size in a switch, a third detrend in a table or a kernel named outside its table
    changes the product (or trips the count of names)."""
    text = _src("spec.hip")
    more = text.replace("case 8192: rc = spec8_launch<8192>(h, a, st); break;",
                        "case 8192: rc = spec8_launch<8192>(h, a, st); break;\n"
                        "        case 16384: rc = spec8_launch<16384>(h, a, st); break;")
    assert more != text and len(C.compiled_instances(more)) == 150 + 12
    with pytest.raises(AssertionError):
        C.compiled_instances(text + "\nstatic auto extra = mix::specmix_kernel<0, false, 2048>;\n")


def test_planner_constants_match_the_sources():
    mixh, splith, spec = _src("specmix.h"), _src("specsplit.h"), _src("spec.hip")
    assert f"constexpr int kMaxPass = {C.K_MAX_PASS};" in mixh
    assert f"constexpr int kMaxM = {C.K_MAX_M};" in mixh
    assert f"constexpr int kMaxSplitLocal = {C.K_MAX_SPLIT_LOCAL};" in splith
    assert f"constexpr int kMaxSplitR0 = {C.K_MAX_SPLIT_R0};" in splith
    assert "return M <= 640 ? 64 : M <= 1280 ? 128 : M <= 2560 ? 256 : M <= 5120 ? 512 : 1024;" in spec
    assert spec.count("int64_t R = (nseg * h->nch) / 2048;") == 1                 # mix
    assert spec.count("int64_t R = (nseg * h->nch * NW) / 2048;") == 1            # split
    assert spec.count("int64_t R = (nitem * h->nch) / 2048;") == 1                # blue
    assert spec.count("int64_t R = (npairs * h->nch) / 2048;") == 1               # fft8
    assert spec.count("int64_t R = (npairs * h->nch) / 512;") == 1                # cube
    assert spec.count("if (R > 64) R = 64;") == 4 and spec.count("if (R > 32) R = 32;") == 1
    assert "kSpecMaxElems = (int64_t)1 << 27;" in spec
    for r in (10, 4, 2, 3, 5, 7):
        assert f"take({r});" in spec
    assert re.search(r"take\(10\);\s*take\(4\);\s*take\(2\);\s*take\(3\);\s*take\(5\);\s*take\(7\);", spec)


def test_launch_record_matches_the_binding():
    from openseize_amd import _lib
    assert _lib.SPEC_LAUNCH_SCALARS + ("radix",) == C.FIELDS and _lib.SPEC_FAMILY == C.FAMILIES
    assert _lib.SPEC_LAUNCH_RADIX == C.K_MAX_PASS
    header = open(os.path.join(C.ROOT, "include", "osz_hip.h")).read()
    for i, name in enumerate(_lib.SPEC_FAMILY):
        tag = f"OSZ_SPECK_{name.upper()} = {i}"
        assert tag + "," in header or tag + " " in header, tag
    assert f"#define OSZ_SPEC_LAUNCH_FIELDS {_lib.SPEC_LAUNCH_FIELDS}\n" in header
    assert f"#define OSZ_SPEC_LAUNCH_RECORDS {_lib.SPEC_LAUNCH_RECORDS}\n" in header


def test_planners_on_known_lengths():
    assert C.mix_plan(648) == (4, 3, 3, 3, 3) and C.mix_plan(1260) == (10, 3, 3, 7)
    assert C.mix_plan(20) == (10,) and C.mix_plan(4) == (2,) and C.mix_plan(2) is None and C.mix_plan(22) is None
    assert C.mix_plan(2 * 10209) is None and C.mix_plan(20412) is not None
    assert C.split_plan(20480) == (4, (4, 10, 4, 4, 4, 4)) and C.split_plan(20412) is None
    assert C.split_plan(20790)[0] == 11 and C.split_plan(2 * 10211) is None
    assert [C.blue_m(n) for n in (2, 256, 257, 513, 2049, 4096)] == [512, 512, 1024, 2048, 8192, 8192]
    r = C.route
    assert r(4096, 4096, 2048).family == "cube" and r(4096, 4096, 2048, {"OSZ_SPEC_FUSED": "0"}).family == "fft8"
    assert r(4096, 4096, 2048, {"OSZ_SPEC_FUSED": "0", "OSZ_SPEC_V8": "0"}).family == "mix"
    assert r(4096, 4096, 2048, {"OSZ_SPEC_FUSED": "0", "OSZ_SPEC_V8": "0", "OSZ_SPEC_MIX": "0"}).family == "staged"
    assert r(4095, 4096, 7) == C.Route("fft8", 4096, 0, (), 0, 0) and r(256, 256, 128).family == "mix"
    assert r(347, 347, 100) == C.Route("blue", 1024, -1, (), 0, 0) and r(4099, 4099, 1).family == "staged"
    assert r(16384, 16384, 8192) == C.Route("mix", 1024, 1, C.mix_plan(16384), 0, 0)


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_case_launches(case):
    """The restated planners send the case to the instance it is there for, and its pushes have
    the shape their kind promises."""
    plan = C.plan_pushes(case)
    recs = [r for _, rs in plan for r in rs]
    assert recs and all(tuple(r) == C.FIELDS for r in recs)
    assert all(C.instance_of(r) == case.want for r in recs), (case.want, recs)
    assert sum(s for s, _ in plan) == C.total_segments(case)
    assert sum(r["nseg"] for r in recs) == C.total_segments(case)
    fam = case.want[0]
    pairs = fam in ("cube", "fft8", "blue")
    if fam in ("cube", "fft8"):
        assert case.want[4] == recs[0]["half"]
    if case.kind == "runs":
        (rec,) = recs
        assert rec["R"] >= 2 and rec["nruns"] >= 2 and rec["head"] in (0, -1)
        items = (rec["nseg"] + 1) // 2 if pairs else rec["nseg"]
        # (all five kernels cut their items into nruns runs the same way: run q covers
        # [q items / nruns, (q + 1) items / nruns) -- p0 / p1 and s0 / s1 in spec.hip, specmix.h, specsplit.h)
        lens = {(q + 1) * items // rec["nruns"] - q * items // rec["nruns"] for q in range(rec["nruns"])}
        assert len(lens) > 1 and max(lens) >= 2, lens           # runs of unequal length, one of R at least
        assert not pairs or rec["nseg"] % 2 == 1                # the last pair is half empty
        if fam in ("mix", "split"):
            assert rec["half"] == case.halfcarry
            assert not case.halfcarry or max(lens) >= 3         # a carried sum of a carried sum
    elif len(case.pushes) > 2 and case.nwin > 8:
        segs = [s for s, _ in plan]
        assert segs[0] == 0 and {s % 2 for s in segs if s} == {0, 1}
        if fam not in ("cube", "staged"):
            heads = [[r["head"] for r in rs] for _, rs in plan if rs]
            assert [1, 0] in heads and [1] in heads and max(len(h) for h in heads) == 2


def test_reference_matches_scipy_signal():
    """The long-double reference against scipy.signal on a float64 copy: detrend, the segments of
    stft (scaled by 1 / sum w) and welch's 'spectrum' average (by 1 / (sum w)^2), to 1e-13."""
    import scipy.signal as sps
    for name in ("fft8-512-half-m2-lin-ragged", "mix-128-n1296-m2-const-ragged", "blue-pad201of347-m2-lin-extra",
                 "blue-1024-n257-m2-lin-ragged"):
        case = next(c for c in C.CASES if c.name == name)
        x, w = C.signal(case), C.window(case)
        kind = "linear" if case.linear else "constant"
        rows = C._detrended(C.segment_rows(x, case, C.LD), w, case.linear, C.LD)
        want = sps.detrend(C.segment_rows(x, case, np.float64), axis=-1, type=kind) * w
        assert float(np.abs(rows - want).max() / np.abs(want).max()) < 1e-13
        X = C.spectrum(x, case, C.LD)
        _, _, Z = sps.stft(x, window=w, nperseg=case.nwin, noverlap=case.nwin - case.stride, nfft=case.nfft,
                           detrend=kind, boundary=None, padded=False, return_onesided=True)
        Z = np.moveaxis(Z, -1, 0) * (w.sum() * C.SCALE)
        assert Z.shape == X.shape
        assert C.row_metric(Z, X, C.DFT).max() < 1e-13
        _, Pw = sps.welch(x, window=w, nperseg=case.nwin, noverlap=case.nwin - case.stride, nfft=case.nfft,
                          detrend=kind, scaling="spectrum", return_onesided=True)
        mean = C.power(X, case.nfft).mean(axis=0)
        assert C.row_metric(Pw * (w.sum() * C.SCALE) ** 2, mean, C.MEAN).max() < 1e-13


def test_metric_is_per_row():
    """One bad bin of one row shows at its own row's scale, however large the other rows are."""
    rng = np.random.default_rng(3)
    ref = (rng.standard_normal((4, 3, 33)) + 1j * rng.standard_normal((4, 3, 33))).astype(np.complex256)
    ref[0] *= 1e6
    got = ref.astype(np.complex128)
    got[2, 1, 7] *= 1 + 1e-6
    m = C.row_metric(got, ref, C.DFT)
    assert m.shape == (4, 3) and m[2, 1] > 1e-7 and np.delete(m.ravel(), 7).max() < 1e-15
    zero = np.zeros((2, 5), C.LD)
    assert C.row_metric(np.zeros((2, 5)), zero, C.PSD).max() == 0 and np.isinf(C.row_metric(np.ones((2, 5)), zero, C.PSD)).all()


@pytest.mark.parametrize("case", [c for c in C.CASES if not c.zero], ids=[c.name for c in C.CASES if not c.zero])
def test_case_inputs_and_e64(case):
    """In every row the DC, first and (even nfft) Nyquist bins hold at least 1 % of the row's mean
    power; with linear detrend the fitted line changes every row's spectrum by more than 1e-3 of
    its rms; e64 lies within a factor 2 of the value recorded for the case."""
    x = C.signal(case)
    X64 = C.spectrum(x, case, np.float64)
    share, change = C.input_conditions(case, x, X64)
    ref = C.reference(case, x, X64)
    rec = C.E64[case.name]
    print(f"{case.name}: share {share:.3g} change {change:.3g} e64 {ref.e64:.3g}")
    assert share >= 0.01 and change > 1e-3
    assert rec / 2 <= ref.e64 <= rec * 2, (ref.e64, rec)


def test_zero_cases_are_zero():
    for case in C.CASES:
        if case.zero:
            assert case.nwin == 1 and not case.linear
            assert not np.any(C.reference(case).exact)
