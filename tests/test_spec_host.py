"""The host tables of the spectral FIR -> cascade kernel (openseize_amd/csrc/spec_tables.h,
used by chain_spec.hip), built by g++ from the same header and (1) held against NumPy,
(2) driven through a NumPy restatement of the kernel's dataflow -- whole pairs with the
overlap add and the mode bursts, the opening pair's carry, the generic closing pair, runs
with a one-pair pre-roll -- against scipy's sosfilt(convolve(x, h)): the block algorithm
and its tables are pinned without a GPU."""

import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.signal as sps

from chain_cells import N, Model, ModelSpecN, ModelZp, ModelZpn, tables, tables_zp  # (the readers and the models)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "host", "spec_host_check.cpp")
    inc = os.path.join(ROOT, "openseize_amd", "csrc")
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "spec_host_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", inc, src, "-o", path])
    return path


CASES = [
    ("butter6 band-pass, 1024 taps (cfg-3)", 1024, sps.butter(6, [0.05, 0.3], "bandpass", output="sos")),
    ("butter6 band-pass, 300 taps", 300, sps.butter(6, [0.05, 0.3], "bandpass", output="sos")),
    ("cheby1 band-pass, 777 taps", 777, sps.cheby1(3, 1, [0.16, 0.48], "bandpass", output="sos")),
    ("butter5 low-pass (a real pole), 513 taps", 513, sps.butter(5, 0.3, output="sos")),
    ("elliptic high-pass, 64 taps", 64, sps.ellip(4, 0.5, 50, 0.25, "highpass", output="sos")),
]


@pytest.mark.parametrize("name,ntaps,sos", CASES, ids=[c[0] for c in CASES])
def test_tables_and_block_algorithm(exe, name, ntaps, sos):
    taps = sps.firwin(ntaps, 0.2)
    T = tables(exe, taps, sos)
    assert T["eligible"], name
    NR, NM, R = T["NR"], T["NM"], T["R"]
    assert NR == min((3841 - ntaps) // 256, 15) and 1 <= R <= min(16 - NR, 2 * NR - 16, 5)
    # (1) against NumPy: the composite spectrum and the mode powers
    w, h = sps.sosfreqz(sos, worN=N, whole=True)
    Hc = np.fft.fft(taps, N) * h / N
    H = T["H"].reshape(N, 2)
    assert np.max(np.abs(H[:, 0] + 1j * H[:, 1] - Hc)) < 1e-15 * np.max(np.abs(Hc)) * 50
    P = T["P"].reshape(32, NM, 2)
    lam = P[17, :, 0] + 1j * P[17, :, 1]
    assert np.all(np.abs(lam[:T["nm"]]) < 1) and np.all(lam[T["nm"]:] == 0)
    poles = np.concatenate([np.roots(s[3:]) for s in sos if s[4] or s[5]])
    for q in range(T["nm"]):
        assert np.min(np.abs(poles - lam[q])) < 1e-12
    assert np.allclose(P[3, :T["nm"], 0] + 1j * P[3, :T["nm"], 1], lam[:T["nm"]] ** 48, rtol=1e-13, atol=0)
    L = T["L"].reshape(5, NM, 2)
    assert np.allclose(L[2, :T["nm"], 0] + 1j * L[2, :T["nm"], 1], lam[:T["nm"]] ** 512, rtol=1e-12, atol=1e-300)
    # (2) the block algorithm with these tables against scipy
    rng = np.random.default_rng(len(taps))
    m = Model(T, ntaps)
    S = m.S
    lens = [2 * S * 5 + 1024, 2 * S * 4, 2 * S * 3 + S + 17, 2 * S + 5, 2 * S * 3 + 2 * S - 1]
    x = rng.standard_normal(sum(lens))
    u = np.convolve(x, taps)
    zi0 = sps.sosfilt_zi(sos) * u[0]
    ref, _ = sps.sosfilt(sos, u, zi=zi0)
    # import: the pending FIR tail (none yet) through the cascade from its state
    carry = np.zeros(7680)
    carry[:m.CL] = sps.sosfilt(sos, np.zeros(m.CL), zi=zi0)[0]
    o, scale = 0, np.max(np.abs(ref))
    for k, n in enumerate(lens):
        f, carry = m.chunk(x[o:o + n], carry, nruns=[1, 2, 3, 4, 2][k])
        assert np.max(np.abs(f - ref[o:o + n])) < 1e-12 * scale, (name, k)
        o += n
    # the carry IS the stream's future if the input stops: the flush of the chain
    assert np.max(np.abs(carry[:ntaps - 1] - ref[o:o + ntaps - 1])) < 1e-12 * scale


def test_what_the_scheme_does_not_take(exe):
    """Cascades outside the scheme are refused (chain_kernel serves them): a double pole,
    ringing that outlasts the guard rows, a filter too long for row 15 to be free, a
    cascade that does not forget."""
    bp = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    assert tables(exe, sps.firwin(1024, 0.2), bp)["eligible"]
    twice = np.vstack([sps.butter(2, 0.2, output="sos")] * 2)          # every pole twice
    assert not tables(exe, sps.firwin(256, 0.2), twice)["eligible"]
    narrow = sps.butter(4, [0.0002, 0.0016], "bandpass", output="sos")  # 0.5-4 Hz at 5 kHz
    assert not tables(exe, sps.firwin(256, 0.2), narrow)["eligible"]
    assert not tables(exe, sps.firwin(1900, 0.2), bp)["eligible"]
    assert not tables(exe, sps.firwin(1024, 0.2), bp, forgets=False)["eligible"]
    assert not tables(exe, sps.firwin(64, 0.2), sps.butter(14, 0.3, output="sos"))["eligible"]   # 7 modes


# ------------------------------------------------------------------ the two-sided scheme
ZP_CASES = [
    ("butter6 band-pass, 1024 taps (cfg-3)", 1024, sps.butter(6, [0.05, 0.3], "bandpass", output="sos")),
    ("butter6 band-pass, 300 taps", 300, sps.butter(6, [0.05, 0.3], "bandpass", output="sos")),
    ("cheby1 band-pass, 777 taps", 777, sps.cheby1(3, 1, [0.16, 0.48], "bandpass", output="sos")),
    ("butter5 low-pass (a real pole), 513 taps", 513, sps.butter(5, 0.3, output="sos")),
]


@pytest.mark.parametrize("name,ntaps,sos", ZP_CASES, ids=[c[0] for c in ZP_CASES])
def test_zero_phase_tables_and_block_algorithm(exe, name, ntaps, sos):
    """FIR -> forward cascade -> backward cascade as one multiplication per bin: the C++
    tables drive the NumPy restatement of chain_zp_kernel against scipy (forward pass from
    sosfilt_zi * u[0], backward pass over the whole stream), every kind of chunk."""
    taps = sps.firwin(ntaps, 0.2)
    T = tables_zp(exe, taps, sos)
    assert T["eligible"], name
    NR, R, Rf = T["NR"], T["R"], T["Rf"]
    assert 8 <= NR <= min((3841 - ntaps) // 256, 15) and 1 <= Rf <= R <= min(16 - NR, 5) and 16 - NR + Rf <= NR
    w, h = sps.sosfreqz(sos, worN=N, whole=True)
    Hc = np.fft.fft(taps, N) * np.abs(h) ** 2 / N
    H = T["H"].reshape(N, 2)
    assert np.max(np.abs(H[:, 0] + 1j * H[:, 1] - Hc)) < 1e-15 * np.max(np.abs(Hc)) * 50
    m = ModelZp(T)
    S, L = m.S, m.L
    rng = np.random.default_rng(ntaps)
    lens = [2 * S * 5 + 1024, 2 * S * 4, 2 * S * 3 + S + 17, 2 * S + 5, 2 * S * 3 + 2 * S - 1, 2 * S * 3 + 300]
    x = rng.standard_normal(sum(lens))
    u = np.convolve(x, taps)
    zi0 = sps.sosfilt_zi(sos) * u[0]
    f, _ = sps.sosfilt(sos, u, zi=zi0)
    ref = sps.sosfilt(sos, np.concatenate([f, np.zeros(8192)])[::-1])[::-1][:len(f)]
    # the stream opens: what the forward start state rings, filtered backwards as well
    zir = sps.sosfilt(sos, np.zeros(7680), zi=zi0)[0]
    carry, held = sps.sosfilt(sos, zir[::-1])[::-1], np.zeros(L)
    out, o = [], 0
    for k, n in enumerate(lens):
        y, carry, held = m.chunk(x[o:o + n], carry, held, nruns=[1, 2, 3, 1, 2, 2][k])
        out.append(y)
        o += n
    got = np.concatenate(out)                     # got[q] is stream sample q - L
    assert np.isfinite(got).all()
    assert np.max(np.abs(got[L:] - ref[:len(got) - L])) < 1e-12 * np.max(np.abs(ref)), name


# ------------------------------------------------- one real block per transform (chain_zpn.hip)
ZPN_CASES = ZP_CASES + [
    ("the identity as the FIR (plain sosfiltfilt)", 2, sps.butter(6, [0.05, 0.3], "bandpass", output="sos")),
    ("cheby1 low-pass, 57 taps", 57, sps.cheby1(5, 1, 0.2, output="sos")),
    ("eight sections (eight modes), 1024 taps", 1024, sps.butter(8, [0.05, 0.3], "bandpass", output="sos")),
    ("Butter [8, 30] / [3, 60] Hz at 500 Hz (SURVEY 8d's class-API cfg-3), 1024 taps", 1024,
     sps.butter(6, [8 / 250, 30 / 250], "bandpass", output="sos")),
    ("a cascade alone whose left tail takes eight rows (blocks of 24)", 2, sps.cheby1(5, 1, 0.2, output="sos")),
]


@pytest.mark.parametrize("name,ntaps,sos", ZPN_CASES, ids=[c[0] for c in ZPN_CASES])
def test_single_block_tables_and_block_algorithm(exe, name, ntaps, sos):
    """The same chain with ONE real block of 8192 samples per transform (odd frequencies,
    negacyclic wrap): tables of spec::build_zpn through the NumPy restatement of
    chain_zpn_kernel against scipy, every kind of chunk."""
    taps = sps.firwin(ntaps, 0.2) if ntaps > 2 else np.array([1.0, 0.0])
    T = tables_zp(exe, taps, sos, mode="zpn")
    assert T["eligible"], name
    NB, R, Rf = T["NR"], T["R"], T["Rf"]
    assert 24 <= NB <= min((7937 - ntaps) // 256, 30) and 1 <= Rf <= R <= min(32 - NB, 8) and 32 - NB + Rf <= NB
    assert T["NS"] in (2, 4, 6) and T["NS"] <= T["NM"] <= 8
    wq = 2 * np.pi * (np.arange(N) + 0.25) / N
    _, h = sps.sosfreqz(sos, worN=wq)
    Hq = np.polyval(taps[::-1], np.exp(-1j * wq)) * np.abs(h) ** 2 / N
    H = T["H"].reshape(N, 2)
    assert np.max(np.abs(H[:, 0] + 1j * H[:, 1] - Hq)) < 1e-12 * np.max(np.abs(Hq))   # (NumPy's polyval is the weak side)
    m = ModelZpn(T)
    S, L = m.S, m.L
    rng = np.random.default_rng(ntaps)
    lens = [S * 5 + 1024, S * 4, S * 3 + S - 17, S + 5, S * 3 + S, S * 3 + 300, 2 * S]
    x = rng.standard_normal(sum(lens))
    u = np.convolve(x, taps)
    zi0 = sps.sosfilt_zi(sos) * u[0]
    f, _ = sps.sosfilt(sos, u, zi=zi0)
    ref = sps.sosfilt(sos, np.concatenate([f, np.zeros(32768)])[::-1])[::-1][:len(f)]
    zir = sps.sosfilt(sos, np.zeros(7680), zi=zi0)[0]
    carry, held = sps.sosfilt(sos, zir[::-1])[::-1], np.zeros(L)
    out, o = [], 0
    for k, n in enumerate(lens):
        y, carry, held = m.chunk(x[o:o + n], carry, held, nruns=[1, 2, 3, 1, 2, 2, 1][k])
        out.append(y)
        o += n
    got = np.concatenate(out)
    assert np.isfinite(got).all()
    # the fit's conditioning sets the floor: the transform's rounding reaches the amplitudes
    # multiplied by about 1 / ratio (spec::build_zpn admits ratio > 3e-7)
    tol = max(3e-12, 1e-16 / T["ratio"])
    assert tol < 4e-10 and np.max(np.abs(got[L:] - ref[:len(got) - L])) < tol * np.max(np.abs(ref)), name


# ------------------------------------- the forward chain on one real block per transform
SPECN_CASES = CASES + [("eight sections, 1024 taps", 1024, sps.butter(8, [0.05, 0.3], "bandpass", output="sos"))]


@pytest.mark.parametrize("name,ntaps,sos", SPECN_CASES, ids=[c[0] for c in SPECN_CASES])
def test_forward_single_block_tables_and_block_algorithm(exe, name, ntaps, sos):
    """FIR -> forward cascade with one real block of 8192 samples per transform: the tables of
    spec::build_specn through the NumPy restatement of the kernel against scipy's
    sosfilt(convolve(x, h)), every kind of chunk, the carry across chunks and as the flush."""
    taps = sps.firwin(ntaps, 0.2)
    T = tables_zp(exe, taps, sos, mode="specn")
    assert T["eligible"], name
    NB, Rf = T["NR"], T["Rf"]
    assert 24 <= NB <= min((7937 - ntaps) // 256, 30) and 1 <= Rf <= 5 and 32 - NB + Rf <= NB
    wq = 2 * np.pi * (np.arange(N) + 0.25) / N
    _, h = sps.sosfreqz(sos, worN=wq)
    Hq = np.polyval(taps[::-1], np.exp(-1j * wq)) * h / N
    H = T["H"].reshape(N, 2)
    assert np.max(np.abs(H[:, 0] + 1j * H[:, 1] - Hq)) < 1e-12 * np.max(np.abs(Hq))
    m = ModelSpecN(T)
    S = m.S
    rng = np.random.default_rng(len(taps))
    lens = [S * 5 + 1024, S * 4, S * 3 + S - 17, S + 5, S * 3 + S, 2 * S]
    x = rng.standard_normal(sum(lens))
    u = np.convolve(x, taps)
    zi0 = sps.sosfilt_zi(sos) * u[0]
    ref, _ = sps.sosfilt(sos, u, zi=zi0)
    carry = np.zeros(7680)
    cl = 4096 + 256 * Rf
    carry[:cl] = sps.sosfilt(sos, np.zeros(cl), zi=zi0)[0]
    o, scale = 0, np.max(np.abs(ref))
    tol = max(1e-12, 1e-16 / T["ratio"])
    for k, n in enumerate(lens):
        f, carry = m.chunk(x[o:o + n], carry, nruns=[1, 2, 3, 1, 2, 1][k])
        assert np.max(np.abs(f - ref[o:o + n])) < tol * scale, (name, k)
        o += n
    assert np.max(np.abs(carry[:ntaps - 1] - ref[o:o + ntaps - 1])) < tol * scale
