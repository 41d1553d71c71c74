"""The compiled instances ("cells") of the FIR -> IIR chain kernels and what tests them.

A cell is one template instance: ("zpn", NB, NM, NS, RM) chain_zpn_kernel<.., true> (zero phase,
one block per transform), ("fwd", NB, NM, NS) chain_zpn_kernel<.., 5, false> (forward chain),
("zp", NR, NM) chain_zp_kernel (zero-phase pair fallback), ("spec", NR, NM) chain_spec_kernel
(forward pair fallback), ("scan", NR, V2) chain_kernel (the cascade as a scan in time).  CORPUS
holds one (FIR, scipy design) pair per reachable cell, written by tests/chain_cell_sweep.py;
UNREACHED names every other instance with the planner's reason.  Shared by
tests/test_chain_cells_host.py (plans and the NumPy dataflow models, no GPU),
tests/test_gpu_chain_cells.py (every cell through the C ABI) and tests/test_spec_host.py /
tests/test_gpu_zp.py (the host-table reader, the models, the stream helpers)."""

import os
import re
import struct
import subprocess
import tempfile
from collections import namedtuple

import numpy as np
import scipy.signal as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


# ----------------------------------------------------------------- the host harness (g++)
_EXE = {}


def build_host_exe():
    """tests/host/spec_host_check.cpp built by g++ from the library's own spec_tables.h (once per
    process)."""
    if "path" not in _EXE:
        src = os.path.join(ROOT, "tests", "host", "spec_host_check.cpp")
        inc = os.path.join(ROOT, "openseize_amd", "csrc")
        path = os.path.join(tempfile.mkdtemp(), "spec_host_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", inc, src, "-o", path])
        _EXE["path"] = path
    return _EXE["path"]


def _write_input(path, taps, sos, forgets):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", len(taps), len(sos), int(forgets)))
        f.write(taps.tobytes())
        f.write(sos.tobytes())


# ------------------------------------------- host tables and the NumPy models of the kernels
def tables(exe, taps, sos, forgets=True):
    taps, sos = np.asarray(taps, np.float64), np.atleast_2d(np.asarray(sos, np.float64))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        _write_input(fin, taps, sos, forgets)
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    elig, NR, NM, nm, R = struct.unpack_from("<iiiii", raw, 0)
    ratio, = struct.unpack_from("<d", raw, 20)
    pos, arrs = 28, []
    for _ in range(4):
        n, = struct.unpack_from("<q", raw, pos)
        arrs.append(np.frombuffer(raw, np.float64, n, pos + 8).copy())
        pos += 8 + 8 * n
    return dict(eligible=bool(elig), NR=NR, NM=NM, nm=nm, R=R, ratio=ratio, H=arrs[0], M=arrs[1],
                P=arrs[2], L=arrs[3])


class Model:
    """The kernel's dataflow (chain_spec.hip) on one channel, with the tables of the C++ build."""

    def __init__(self, T, wlen):
        self.NR, self.NM, self.R = T["NR"], T["NM"], T["R"]
        self.S, self.D = 256 * self.NR, 16 - self.NR
        H = T["H"].reshape(N, 2)
        self.Hc = (H[:, 0] + 1j * H[:, 1]) * N            # the tables carry the 1/4096
        M = T["M"].reshape(2 * self.NM, 64)
        self.M = M[:self.NM] + 1j * M[self.NM:]
        P = T["P"].reshape(32, self.NM, 2)
        P = P[..., 0] + 1j * P[..., 1]
        t = np.arange(256)
        self.P = P[t >> 4] * P[16 + (t & 15)]             # lambda^t as the kernel forms it
        L = T["L"].reshape(5, self.NM, 2)
        self.L = L[..., 0] + 1j * L[..., 1]
        self.CL = N + 256 * self.R

    def window(self, x):
        buf = np.zeros(N)
        buf[:len(x)] = x
        return np.real(np.fft.ifft(np.fft.fft(buf) * self.Hc))

    def fit(self, win):
        return self.M @ win[3840:3904]

    def burst(self, mu, e):
        ok = (e >= 0) & (e < 256 * self.R)
        ee = np.where(ok, e, 0)
        return np.where(ok, np.real((self.L[ee >> 8] * self.P[ee & 255]) @ mu), 0.0)

    def chunk(self, x, carry_in, nruns):
        n, S, NR, D, R = len(x), self.S, self.NR, self.D, self.R
        pair = 2 * S
        npw = n // pair
        rem = n - npw * pair
        W = npw - 1 if rem == 0 else npw
        assert W >= 1
        f = np.full(n, np.nan)
        nruns = max(1, min(nruns, W))
        t = np.arange(256)
        carry_out = None
        for run in range(nruns):
            p0, p1 = run * W // nruns, (run + 1) * W // nruns
            cr, mu_prev = np.zeros((D, 256)), np.zeros(self.NM, complex)
            for p in range(p0 if run == 0 else p0 - 1, p1):
                o = p * pair
                wa, wb = self.window(x[o:o + S]), self.window(x[o + S:o + pair])
                mu_a, mu_b = self.fit(wa), self.fit(wb)
                Ya, Yb = wa.reshape(16, 256), wb.reshape(16, 256)
                A, B = Ya[:NR].copy(), Yb[:NR].copy()
                A[:D] += cr
                B[:D] += Ya[NR:]
                cr = Yb[NR:].copy()
                for r in range(R):
                    A[r] += self.burst(-mu_a, 256 * r + t)
                    A[D + r] += self.burst(mu_prev, 256 * r + t)
                    B[r] += self.burst(-mu_b, 256 * r + t)
                    B[D + r] += self.burst(mu_a, 256 * r + t)
                mu_prev = mu_b
                if p == 0:
                    ci = np.zeros(pair)
                    ci[:self.CL] = carry_in[:self.CL]
                    A += ci[:S].reshape(NR, 256)
                    B += ci[S:].reshape(NR, 256)
                if p >= p0:
                    f[o:o + S], f[o + S:o + pair] = A.ravel(), B.ravel()
            if run == nruns - 1:
                o = W * pair
                la = min(n - o, S)
                lb = n - o - la
                wa, wb = self.window(x[o:o + la]), self.window(x[o + la:o + la + lb])
                mu_a, mu_b = self.fit(wa), self.fit(wb)
                acc, i = np.zeros(8192), np.arange(8192)
                acc[:256 * D] += cr.ravel()
                acc[:N] += wa
                acc[la:la + N] += wb
                for mu, off in ((mu_prev, 256 * D), (-mu_a, 0), (-mu_b, la), (mu_a, N), (mu_b, la + N)):
                    acc += self.burst(mu, i - off)
                f[o:n] = acc[:la + lb]
                carry_out = np.zeros(7680)
                seg = acc[la + lb:]
                carry_out[:min(len(seg), 7680)] = seg[:7680]
        return f, carry_out



def tables_zp(exe, taps, sos, forgets=True, mode="zp"):
    taps, sos = np.asarray(taps, np.float64), np.atleast_2d(np.asarray(sos, np.float64))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        _write_input(fin, taps, sos, forgets)
        subprocess.check_call([exe, fin, fout, mode])
        raw = open(fout, "rb").read()
    elig, NR, NM, nm, R, nh, Rf, NS = struct.unpack_from("<iiiiiiii", raw, 0)
    ratio, = struct.unpack_from("<d", raw, 32)
    pos, arrs = 40, []
    for _ in range(4):
        n, = struct.unpack_from("<q", raw, pos)
        arrs.append(np.frombuffer(raw, np.float64, n, pos + 8).copy())
        pos += 8 + 8 * n
    return dict(eligible=bool(elig), NR=NR, NM=NM, nm=nm, R=R, Rf=Rf, nh=nh, NS=NS, ratio=ratio, H=arrs[0],
                M=arrs[1], P=arrs[2], L=arrs[3])


class ModelZp:
    """The dataflow of chain_zp_kernel on one channel with the tables of the C++ build:
    whole pairs (overlap add, four forward and four backward bursts, the last R rows of
    block b held back until the next pair's block a has been fitted), runs that start one
    pair early and store that pair's held rows for the run before, the opening pair (carry, held samples of the previous chunk), the
    generic closing pair, outputs delayed by L = 256 R samples."""

    def __init__(self, T):
        self.NR, self.NM, self.R, self.Rf, self.nh = T["NR"], T["NM"], T["R"], T["Rf"], T["nh"]
        self.S, self.D, self.L = 256 * self.NR, 16 - self.NR, 256 * T["R"]
        H = T["H"].reshape(N, 2)
        self.Hc = (H[:, 0] + 1j * H[:, 1]) * N
        M = T["M"].reshape(4 * self.NM, 2 * self.nh)
        self.Mmu = M[:self.NM] + 1j * M[self.NM:2 * self.NM]
        self.Mnu = M[2 * self.NM:3 * self.NM] + 1j * M[3 * self.NM:]
        P = T["P"].reshape(20, self.NM, 2)
        P = P[..., 0] + 1j * P[..., 1]
        t = np.arange(256)
        self.P = P[t >> 5] * P[8 + ((t >> 2) & 7)] * P[16 + (t & 3)]     # lambda^t as the kernel forms it
        Lr = T["L"].reshape(5, self.NM, 2)
        self.Lr = Lr[..., 0] + 1j * Lr[..., 1]
        self.lsel = np.concatenate([np.arange(self.nh), np.arange(256 - self.nh, 256)])

    def window(self, x):
        buf = np.zeros(N)
        buf[:len(x)] = x
        return np.real(np.fft.ifft(np.fft.fft(buf) * self.Hc))

    def fit(self, win):
        y = win[3840 + self.lsel]
        return self.Mmu @ y, self.Mnu @ y

    def burst(self, amp, e, rows):
        ok = (e >= 0) & (e < 256 * rows)
        ee = np.where(ok, e, 0)
        return np.where(ok, np.real((self.Lr[ee >> 8] * self.P[ee & 255]) @ amp), 0.0)

    def chunk(self, x, carry_in, held_in, nruns):
        n, S, NR, D, R, L, Rf = len(x), self.S, self.NR, self.D, self.R, self.L, self.Rf
        pair = 2 * S
        npw = n // pair
        rem = n - npw * pair
        W = npw - 1 if rem == 0 else npw
        assert W >= 1
        lc = n - W * pair
        y, held_out = np.full(n, np.nan), np.full(L, np.nan)
        t = np.arange(256)

        def put(i, v):
            q = i + L
            m = q < n
            y[q[m]] = v[m]
            m2 = (~m) & (i < n)
            held_out[q[m2] - n] = v[m2]

        F = lambda amp, r: self.burst(amp, 256 * r + t, Rf)            # forward burst, row r (Rf rows)
        Bk = lambda amp, r: self.burst(amp, 256 * r + 255 - t, R)      # backward burst, r-th row down (R rows)
        nruns = max(1, min(nruns, W))
        carry_out = None
        for run in range(nruns):
            p0, p1 = run * W // nruns, (run + 1) * W // nruns
            first = p0 if run == 0 else p0 - 1
            lastf = p1 - 1
            cr = np.zeros((D, 256))
            mu_pb = nu_pb = np.zeros(self.NM, complex)
            held = None
            for p in range(first, lastf + 1):
                o = p * pair
                wa, wb = self.window(x[o:o + S]), self.window(x[o + S:o + pair])
                (mu_a, nu_a), (mu_b, nu_b) = self.fit(wa), self.fit(wb)
                Ya, Yb = wa.reshape(16, 256), wb.reshape(16, 256)
                A, B = Ya[:NR].copy(), Yb[:NR].copy()
                A[:D] += cr
                B[:D] += Ya[NR:]
                cr = Yb[NR:].copy()
                for r in range(R):
                    A[r] += F(-mu_a, r)
                    A[D + r] += F(mu_pb, r)
                    A[D - 1 - r] += Bk(-nu_pb, r)
                    A[NR - 1 - r] += Bk(nu_b, r)
                    B[r] += F(-mu_b, r)
                    B[D + r] += F(mu_a, r)
                    B[D - 1 - r] += Bk(-nu_a, r)
                if p == 0:
                    ci = np.zeros(pair)
                    ci[:len(carry_in)] = carry_in[:pair]
                    A += ci[:S].reshape(NR, 256)
                    B += ci[S:].reshape(NR, 256)
                if held is not None:
                    # (also the rows of the pair a run starts early with: its block b depends
                    # on nothing before it, and the run before leaves them to this one)
                    for r in range(R):
                        held[r] += Bk(nu_a, r)
                        put((p - 1) * pair + S + 256 * (NR - 1 - r) + t, held[r])
                elif p == 0:
                    for rr in range(R):
                        y[256 * rr + t] = held_in[256 * rr + t] + Bk(nu_a, R - 1 - rr)
                if p0 <= p < p1:
                    for j in range(NR):
                        put(o + 256 * j + t, A[j])
                    for j in range(NR - R):
                        put(o + S + 256 * j + t, B[j])
                held = [B[NR - 1 - r].copy() for r in range(R)]
                mu_pb, nu_pb = mu_b, nu_b
            if run == nruns - 1:
                o = W * pair
                la = min(lc, S)
                lb = lc - la
                wa, wb = self.window(x[o:o + la]), self.window(x[o + la:o + la + lb])
                (mu_a, nu_a), (mu_b, nu_b) = self.fit(wa), self.fit(wb)
                for r in range(R):
                    held[r] += Bk(nu_a, r)
                    put((W - 1) * pair + S + 256 * (NR - 1 - r) + t, held[r])
                acc, i = np.zeros(8192), np.arange(8192)
                acc[:256 * D] += cr.ravel()
                acc[:N] += wa
                acc[la:la + N] += wb
                for amp, off in ((mu_pb, 256 * D), (-mu_a, 0), (-mu_b, la), (mu_a, N), (mu_b, la + N)):
                    acc += self.burst(amp, i - off, Rf)
                for amp, e0 in ((-nu_pb, 256 * D - 1), (-nu_a, N - 1), (-nu_b, la + N - 1), (nu_b, la - 1)):
                    acc += self.burst(amp, e0 - i, R)
                put(o + i[:lc], acc[:lc])
                carry_out = np.zeros(7680)
                seg = acc[lc:]
                carry_out[:min(len(seg), 7680)] = seg[:7680]
        return y, carry_out, held_out



MW = 8192


class ModelZpn:
    """The dataflow of chain_zpn_kernel on one channel with the tables of the C++ build: a window
    of 8192 samples per block through the 4096-point transform at the odd frequencies (fft::nega:
    negacyclic wrap), the fit on row 31, the in-window corrections ADDED (the wrap changes the
    sign), the right tail's continuation from the previous block's amplitudes, the last R rows
    of a block held back until the next block has been fitted, runs that start one block early,
    the opening block (carry, held samples of the previous chunk), the generic closing block
    (window in an accumulator of 8192, the burst behind it straight into the carry), outputs
    delayed by L = 256 R samples."""

    def __init__(self, T):
        self.NB, self.NM, self.R, self.Rf, self.nh = T["NR"], T["NM"], T["R"], T["Rf"], T["nh"]
        self.NS = NS = T["NS"]
        self.S, self.D, self.L = 256 * self.NB, 32 - self.NB, 256 * T["R"]
        H = T["H"].reshape(N, 2)
        self.Hq = (H[:, 0] + 1j * H[:, 1]) * N
        M = T["M"].reshape(2 * NS + 2 * self.NM, 2 * self.nh)
        self.Mmu = M[:NS] + 1j * M[NS:2 * NS]                        # the slow modes' right tails only
        self.Mnu = M[2 * NS:2 * NS + self.NM] + 1j * M[2 * NS + self.NM:]
        P = T["P"].reshape(20, self.NM, 2)
        P = P[..., 0] + 1j * P[..., 1]
        t = np.arange(256)
        self.P = P[t >> 5] * P[8 + ((t >> 2) & 7)] * P[16 + (t & 3)]
        Lr = T["L"].reshape(-1, self.NM, 2)                            # (eight rows: spec::kRMaxN)
        self.Lr = Lr[..., 0] + 1j * Lr[..., 1]
        self.lsel = np.concatenate([np.arange(self.nh), np.arange(256 - self.nh, 256)])
        self.tw = np.exp(-1j * np.pi * np.arange(N) / MW)

    def window(self, x):
        buf = np.zeros(MW)
        buf[:len(x)] = x
        z = (buf[:N] - 1j * buf[N:]) * self.tw
        w = np.fft.ifft(np.fft.fft(z) * self.Hq) * np.conj(self.tw)
        return np.concatenate([w.real, -w.imag])

    def fit(self, win):
        y = win[MW - 256 + self.lsel]
        return self.Mmu @ y, self.Mnu @ y

    def burst(self, amp, e, rows):
        """Re sum_q amp_q lambda_q^e over the modes `amp` names -- mu: the NS slow ones; nu: all NM
        in its first row of 256 samples, the slow ones behind it"""
        ok = (e >= 0) & (e < 256 * rows)
        ee = np.where(ok, e, 0)
        nq = len(amp)
        terms = (self.Lr[ee >> 8, :nq] * self.P[ee & 255, :nq]) * amp
        if nq > self.NS:
            terms[ee >= 256, self.NS:] = 0.0
        return np.where(ok, np.real(terms.sum(-1)), 0.0)

    def chunk(self, x, carry_in, held_in, nruns):
        n, S, NB, D, R, L, Rf = len(x), self.S, self.NB, self.D, self.R, self.L, self.Rf
        W = (n - 1) // S                       # whole blocks; the closing block has 1 .. S samples
        assert W >= 1
        lc = n - W * S
        y, held_out = np.full(n, np.nan), np.full(L, np.nan)
        t = np.arange(256)

        def put(i, v):
            q = i + L
            m = q < n
            y[q[m]] = v[m]
            m2 = (~m) & (i < n)
            held_out[q[m2] - n] = v[m2]

        F = lambda amp, r: self.burst(amp, 256 * r + t, Rf)
        Bk = lambda amp, r: self.burst(amp, 256 * r + 255 - t, R)
        nruns = max(1, min(nruns, W))
        carry_out = None
        for run in range(nruns):
            p0, p1 = run * W // nruns, (run + 1) * W // nruns
            first, lastf = (p0 if run == 0 else p0 - 1), p1 - 1
            cr = np.zeros((D, 256))
            mu_p = np.zeros(self.NS, complex)
            held = None
            for p in range(first, lastf + 1):
                o = p * S
                win = self.window(x[o:o + S])
                mu, nu = self.fit(win)
                Y = win.reshape(32, 256).copy()
                for r in range(Rf):
                    Y[r] += F(mu, r)                # the wrapped right tail (sign changed) leaves the window
                for r in range(R):
                    Y[31 - r] += Bk(nu, r)          # and the wrapped left tail
                A = Y[:NB].copy()
                A[:D] += cr
                cr = Y[NB:].copy()
                for r in range(Rf):
                    A[D + r] += F(mu_p, r)          # the previous block's right tail continues here
                if p == 0:
                    ci = np.zeros(S)
                    m = min(len(carry_in), S)
                    ci[:m] = carry_in[:m]
                    A += ci.reshape(NB, 256)
                if held is not None:
                    for r in range(R):
                        held[r] += Bk(nu, r)
                        put((p - 1) * S + 256 * (NB - 1 - r) + t, held[r])
                elif p == 0:
                    for rr in range(R):
                        y[256 * rr + t] = held_in[256 * rr + t] + Bk(nu, R - 1 - rr)
                if p0 <= p < p1:
                    for j in range(NB - R):
                        put(o + 256 * j + t, A[j])
                held = [A[NB - 1 - r].copy() for r in range(R)]
                mu_p = mu
            if run == nruns - 1:
                o, la = W * S, lc
                win = self.window(x[o:o + la])
                mu, nu = self.fit(win)
                for r in range(R):
                    held[r] += Bk(nu, r)
                    put((W - 1) * S + 256 * (NB - 1 - r) + t, held[r])
                i = np.arange(MW)
                acc = win.copy()
                acc[:256 * D] += cr.ravel()
                acc += self.burst(mu_p, i - 256 * D, Rf)
                acc += self.burst(mu, i, Rf)
                acc += self.burst(nu, MW - 1 - i, R)
                put(o + i[:lc], acc[:lc])
                k = np.arange(7680)
                src = lc + k
                carry_out = np.where(src < MW, acc[np.minimum(src, MW - 1)], self.burst(mu, src - MW, Rf))
        return y, carry_out, held_out



class ModelSpecN:
    """FIR -> sosfilt (no backward pass) with the tables of spec::build_specn: the causal half of
    ModelZpn -- the right tail wraps with its sign changed and is added back in the window,
    continues into the next block from the previous block's amplitudes; no lag, nothing held."""

    def __init__(self, T):
        self.NB, self.NM, self.NS, self.Rf, self.nh = T["NR"], T["NM"], T["NS"], T["Rf"], T["nh"]
        self.S, self.D = 256 * self.NB, 32 - self.NB
        H = T["H"].reshape(N, 2)
        self.Hq = (H[:, 0] + 1j * H[:, 1]) * N
        M = T["M"].reshape(2 * self.NS, 2 * self.nh)
        self.Mmu = M[:self.NS] + 1j * M[self.NS:]
        P = T["P"].reshape(20, self.NM, 2)
        P = P[..., 0] + 1j * P[..., 1]
        t = np.arange(256)
        self.P = P[t >> 5] * P[8 + ((t >> 2) & 7)] * P[16 + (t & 3)]
        Lr = T["L"].reshape(-1, self.NM, 2)
        self.Lr = Lr[..., 0] + 1j * Lr[..., 1]
        self.lsel = np.concatenate([np.arange(self.nh), np.arange(256 - self.nh, 256)])
        self.tw = np.exp(-1j * np.pi * np.arange(N) / MW)

    def window(self, x):
        buf = np.zeros(MW)
        buf[:len(x)] = x
        z = (buf[:N] - 1j * buf[N:]) * self.tw
        w = np.fft.ifft(np.fft.fft(z) * self.Hq) * np.conj(self.tw)
        return np.concatenate([w.real, -w.imag])

    def burst(self, amp, e):
        ok = (e >= 0) & (e < 256 * self.Rf)
        ee = np.where(ok, e, 0)
        nq = len(amp)
        return np.where(ok, np.real(((self.Lr[ee >> 8, :nq] * self.P[ee & 255, :nq]) * amp).sum(-1)), 0.0)

    def chunk(self, x, carry_in, nruns):
        n, S, NB, D, Rf = len(x), self.S, self.NB, self.D, self.Rf
        W = (n - 1) // S
        assert W >= 1
        lc = n - W * S
        f = np.full(n, np.nan)
        t = np.arange(256)
        nruns = max(1, min(nruns, W))
        carry_out = None
        for run in range(nruns):
            p0, p1 = run * W // nruns, (run + 1) * W // nruns
            cr, mu_p = np.zeros((D, 256)), np.zeros(self.NS, complex)
            blocks = list(range(p0 if run == 0 else p0 - 1, p1)) + ([W] if run == nruns - 1 else [])
            for p in blocks:
                o = p * S
                la = S if p < W else lc
                win = self.window(x[o:o + la])
                mu = self.Mmu @ win[MW - 256 + self.lsel]
                Y = win.reshape(32, 256).copy()
                Y[:D] += cr
                for r in range(Rf):
                    Y[r] += self.burst(mu, 256 * r + t)
                    Y[D + r] += self.burst(mu_p, 256 * r + t)
                if p == 0:
                    ci = np.zeros(MW)
                    m = min(len(carry_in), MW)
                    ci[:m] = carry_in[:m]
                    Y += ci.reshape(32, 256)
                if p < W:
                    if p >= p0:
                        f[o:o + S] = Y[:NB].ravel()
                    cr, mu_p = Y[NB:].copy(), mu
                else:
                    flat = Y.ravel()
                    f[o:n] = flat[:lc]
                    k = np.arange(7680)
                    src = lc + k
                    carry_out = np.where(src < MW, flat[np.minimum(src, MW - 1)], self.burst(mu, src - MW))
        return f, carry_out


def host_plan(exe, taps, sos, forgets=True):
    """What the planners choose for (taps, sos), as the library builds its tables (harness mode
    `plan`): the zero-phase kernel (2 build_zpn, 1 build_zp, 0 refused) and the forward route
    (2 build_specn, 1 the pair tables, 0 the time scan)."""
    taps, sos = np.asarray(taps, np.float64), np.atleast_2d(np.asarray(sos, np.float64))
    with tempfile.TemporaryDirectory() as tmp:
        fin = os.path.join(tmp, "in.bin")
        _write_input(fin, taps, sos, forgets)
        out = subprocess.check_output([exe, fin, "-", "plan"], text=True).split()
    assert out[0] == "zp" and out[9] == "fwd", out
    z, f = [int(v) for v in out[1:8]], [int(v) for v in out[10:14]]
    return dict(kernel=z[0], rows=z[1], NM=z[2], NS=z[3], R=z[4], Rf=z[5], RM=z[6], zp_ratio=float(out[8]),
                route=f[0], frows=f[1], fNM=f[2], fNS=f[3], fwd_ratio=float(out[14]), ntaps=len(taps),
                nsec=len(sos))


def scan_rows(ntaps):
    """Rows of 256 samples per block of the FIR's single part (fir.hip, fir_build_part); 0 when the
    FIR is partitioned (more than 2048 taps) or has fewer than two."""
    if ntaps < 2 or ntaps > 2048:
        return 0
    return min((N - ntaps + 1) // 256, 15)


def cells_of_plan(p, ntaps=None):
    """[(cell, fit ratio)] of a host plan: its zero-phase cell and its forward cell."""
    out = []
    if p["kernel"] == 2:
        out.append((("zpn", p["rows"], p["NM"], p["NS"], p["RM"]), p["zp_ratio"]))
    elif p["kernel"] == 1:
        out.append((("zp", p["rows"], p["NM"]), p["zp_ratio"]))
    if p["route"] == 2:
        out.append((("fwd", p["frows"], p["fNM"], p["fNS"]), p["fwd_ratio"]))
    elif p["route"] == 1:
        out.append((("spec", p["frows"], p["fNM"]), p["fwd_ratio"]))
    else:
        nr = scan_rows(p["ntaps"])
        if 8 <= nr <= 15:
            out.append((("scan", nr, int(p["nsec"] <= 8)), 1.0))
    return out


# ------------------------------------------------------------------------ recipes and corpus
def fir_taps(ntaps, cutoff=0.2):
    """The FIR of a recipe: firwin(ntaps, cutoff); 2 taps: the identity (plain sosfiltfilt)."""
    return sps.firwin(ntaps, cutoff) if ntaps > 2 else np.array([1.0, 0.0])


def design_sos(kind, order, rip, wn, btype):
    """scipy's `kind`(order, *rip, wn, btype) as second-order sections."""
    return getattr(sps, kind)(order, *rip, wn, btype, output="sos")


# cell, FIR (taps, cut-off), design (kind, order, ripple arguments, Wn, btype), fit ratio of the
# cell's table (1.0 for the time scan, which fits nothing)
Cell = namedtuple("Cell", "cell taps cutoff design ratio")


# 196 cells (179 since build_zpn keeps R + Rf <= 2 NB - 32) from 127600 (FIR, design) pairs (tests/chain_cell_sweep.py; nine
# representatives re-picked by the lowest error of their NumPy model, not the best fit ratio)
CORPUS = [
    Cell(('fwd', 24, 2, 2), 769, 0.2, ('butter', 1, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('fwd', 24, 4, 2), 1650, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 24, 4, 4), 1650, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.262e-01),
    Cell(('fwd', 24, 6, 2), 1650, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 24, 6, 4), 1650, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 24, 6, 6), 1650, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 24, 8, 2), 1650, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 24, 8, 4), 1400, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.764e-01),
    Cell(('fwd', 24, 8, 6), 257, 0.2, ('cheby1', 13, (3.0,), 0.45, 'lowpass'), 3.114e-01),
    Cell(('fwd', 25, 2, 2), 257, 0.2, ('butter', 1, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('fwd', 25, 4, 2), 1400, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 25, 4, 4), 1400, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.262e-01),
    Cell(('fwd', 25, 6, 2), 1400, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 25, 6, 4), 1400, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 25, 6, 6), 1400, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 25, 8, 2), 1400, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 25, 8, 4), 1200, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.764e-01),
    Cell(('fwd', 25, 8, 6), 2, 0.2, ('cheby1', 7, (3.0,), (0.3, 0.6), 'bandstop'), 2.828e-01),
    Cell(('fwd', 26, 2, 2), 2, 0.2, ('butter', 1, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('fwd', 26, 4, 2), 1100, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 26, 4, 4), 1100, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.262e-01),
    Cell(('fwd', 26, 6, 2), 1100, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 26, 6, 4), 1100, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 26, 6, 6), 1100, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 26, 8, 2), 1100, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 26, 8, 4), 900, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.764e-01),
    Cell(('fwd', 26, 8, 6), 33, 0.2, ('cheby1', 7, (3.0,), (0.3, 0.6), 'bandstop'), 2.828e-01),
    Cell(('fwd', 27, 2, 2), 2, 0.2, ('butter', 1, (), 0.004, 'highpass'), 1.000e+00),
    Cell(('fwd', 27, 4, 2), 900, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 27, 4, 4), 640, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.262e-01),
    Cell(('fwd', 27, 6, 2), 900, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 27, 6, 4), 900, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 27, 6, 6), 900, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 27, 8, 2), 900, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 27, 8, 4), 513, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.764e-01),
    Cell(('fwd', 27, 8, 6), 64, 0.2, ('cheby1', 7, (3.0,), (0.3, 0.6), 'bandstop'), 2.828e-01),
    Cell(('fwd', 28, 2, 2), 2, 0.2, ('cheby2', 1, (80.0,), 0.008, 'highpass'), 1.000e+00),
    Cell(('fwd', 28, 4, 2), 640, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 28, 4, 4), 129, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.262e-01),
    Cell(('fwd', 28, 6, 2), 640, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 28, 6, 4), 640, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 28, 6, 6), 513, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 28, 8, 2), 640, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 28, 8, 4), 257, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.764e-01),
    Cell(('fwd', 28, 8, 6), 33, 0.2, ('cheby1', 8, (1.0,), (0.3, 0.6), 'bandstop'), 1.232e-01),
    Cell(('fwd', 29, 2, 2), 2, 0.2, ('cheby1', 1, (0.1,), 0.035, 'highpass'), 1.000e+00),
    Cell(('fwd', 29, 4, 2), 300, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 29, 4, 4), 2, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.262e-01),
    Cell(('fwd', 29, 6, 2), 300, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 29, 6, 4), 2, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 29, 6, 6), 257, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 29, 8, 2), 300, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 29, 8, 4), 129, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.764e-01),
    Cell(('fwd', 29, 8, 6), 400, 0.2, ('butter', 7, (), (0.1, 0.2), 'bandpass'), 3.140e-04),   # (re-picked: lowest model error)
    Cell(('fwd', 30, 2, 2), 2, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('fwd', 30, 4, 2), 2, 0.2, ('cheby1', 5, (3.0,), 0.3, 'lowpass'), 5.054e-01),
    Cell(('fwd', 30, 4, 4), 2, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('fwd', 30, 6, 2), 2, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('fwd', 30, 6, 4), 33, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('fwd', 30, 6, 6), 2, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 3.897e-01),
    Cell(('fwd', 30, 8, 2), 33, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.991e-02),
    Cell(('fwd', 30, 8, 4), 33, 0.2, ('cheby1', 7, (1.0,), (0.3, 0.6), 'bandstop'), 1.578e-01),
    Cell(('fwd', 30, 8, 6), 2, 0.2, ('cheby1', 8, (0.1,), (0.3, 0.6), 'bandpass'), 5.502e-02),
    Cell(('scan', 8, 0), 1850, 0.2, ('butter', 17, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 8, 1), 1850, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 9, 0), 1650, 0.2, ('butter', 17, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 9, 1), 1650, 0.2, ('butter', 1, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('scan', 10, 0), 1400, 0.2, ('butter', 19, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 10, 1), 1400, 0.2, ('butter', 1, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('scan', 11, 0), 1100, 0.2, ('butter', 17, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 11, 1), 1100, 0.2, ('butter', 2, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('scan', 12, 0), 900, 0.2, ('butter', 17, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 12, 1), 900, 0.2, ('butter', 2, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('scan', 13, 0), 640, 0.2, ('butter', 17, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 13, 1), 640, 0.2, ('butter', 2, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('scan', 14, 0), 300, 0.2, ('butter', 19, (), 0.008, 'highpass'), 1.000e+00),
    Cell(('scan', 14, 1), 300, 0.2, ('butter', 2, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('scan', 15, 0), 2, 0.2, ('butter', 17, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('scan', 15, 1), 2, 0.2, ('butter', 2, (), 0.004, 'lowpass'), 1.000e+00),
    Cell(('spec', 9, 6), 1400, 0.2, ('butter', 12, (), 0.1, 'lowpass'), 3.048e-03),
    Cell(('spec', 10, 6), 1100, 0.2, ('butter', 12, (), 0.1, 'lowpass'), 3.048e-03),
    Cell(('spec', 11, 6), 900, 0.2, ('butter', 12, (), 0.1, 'lowpass'), 3.048e-03),
    Cell(('spec', 12, 6), 640, 0.2, ('butter', 12, (), 0.1, 'lowpass'), 3.048e-03),
    Cell(('spec', 13, 6), 300, 0.2, ('butter', 12, (), 0.1, 'lowpass'), 3.048e-03),
    Cell(('spec', 14, 6), 2, 0.2, ('butter', 12, (), 0.1, 'lowpass'), 3.048e-03),
    Cell(('zpn', 22, 4, 2, 12), 2048, 0.2, ('cheby1', 7, (3.0,), 0.2, 'highpass'), 2.430e-01),
    Cell(('zpn', 22, 4, 4, 12), 33, 0.2, ('cheby1', 8, (3.0,), 0.2, 'lowpass'), 3.909e-01),
    Cell(('zpn', 22, 6, 2, 12), 2048, 0.2, ('ellip', 9, (1.0, 80.0), 0.45, 'lowpass'), 1.854e-01),
    Cell(('zpn', 22, 6, 6, 12), 513, 0.2, ('cheby1', 5, (3.0,), (0.2, 0.4), 'bandpass'), 2.529e-02),   # (re-picked: lowest model error)
    Cell(('zpn', 22, 8, 4, 12), 2048, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.647e-01),
    Cell(('zpn', 22, 8, 6, 12), 64, 0.2, ('cheby1', 7, (3.0,), (0.3, 0.6), 'bandstop'), 2.316e-01),
    Cell(('zpn', 23, 2, 2, 12), 1850, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('zpn', 23, 4, 2, 12), 1850, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 23, 4, 4, 12), 1850, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.260e-01),
    Cell(('zpn', 23, 6, 2, 12), 1850, 0.2, ('cheby1', 9, (1.0,), 0.3, 'lowpass'), 2.571e-01),
    Cell(('zpn', 23, 6, 4, 12), 1850, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('zpn', 23, 6, 6, 12), 2, 0.2, ('cheby1', 6, (3.0,), (0.3, 0.6), 'bandpass'), 2.866e-01),   # (re-picked: lowest model error)
    Cell(('zpn', 23, 8, 2, 12), 1850, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.990e-02),
    Cell(('zpn', 23, 8, 4, 12), 1793, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.647e-01),
    Cell(('zpn', 23, 8, 6, 12), 257, 0.2, ('cheby1', 7, (3.0,), (0.3, 0.6), 'bandstop'), 2.316e-01),
    Cell(('zpn', 24, 2, 2, 5), 1650, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('zpn', 24, 2, 2, 8), 2, 0.2, ('cheby2', 1, (40.0,), 0.45, 'lowpass'), 9.991e-01),
    Cell(('zpn', 24, 4, 2, 5), 1650, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 24, 4, 2, 8), 129, 0.2, ('ellip', 8, (0.5, 50.0), 0.45, 'lowpass'), 8.523e-02),   # (re-picked: lowest model error)
    Cell(('zpn', 24, 4, 4, 5), 1650, 0.2, ('cheby1', 3, (3.0,), (0.2, 0.4), 'bandpass'), 4.890e-01),
    Cell(('zpn', 24, 4, 4, 8), 2, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.260e-01),
    Cell(('zpn', 24, 6, 2, 5), 1650, 0.2, ('cheby1', 9, (1.0,), 0.3, 'lowpass'), 2.571e-01),
    Cell(('zpn', 24, 6, 2, 8), 33, 0.2, ('ellip', 9, (1.0, 80.0), 0.45, 'lowpass'), 1.854e-01),
    Cell(('zpn', 24, 6, 4, 5), 1650, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('zpn', 24, 6, 4, 8), 2, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.674e-01),
    Cell(('zpn', 24, 6, 6, 5), 1650, 0.2, ('cheby2', 6, (80.0,), (0.2, 0.4), 'bandpass'), 2.766e-04),
    Cell(('zpn', 24, 6, 6, 8), 2, 0.2, ('ellip', 5, (0.5, 50.0), (0.2, 0.4), 'bandpass'), 1.180e-01),   # (re-picked: lowest model error)
    Cell(('zpn', 24, 8, 2, 5), 1650, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.990e-02),
    Cell(('zpn', 24, 8, 2, 8), 1650, 0.2, ('cheby2', 13, (60.0,), 0.1, 'lowpass'), 9.287e-07),
    Cell(('zpn', 24, 8, 4, 5), 1793, 0.2, ('ellip', 7, (0.1, 70.0), (0.3, 0.6), 'bandstop'), 2.782e-02),   # (re-picked: lowest model error)
    Cell(('zpn', 24, 8, 4, 8), 33, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.647e-01),
    Cell(('zpn', 24, 8, 6, 8), 64, 0.2, ('cheby1', 8, (1.0,), (0.3, 0.6), 'bandstop'), 3.827e-02),
    Cell(('zpn', 25, 2, 2, 5), 1400, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('zpn', 25, 2, 2, 8), 513, 0.2, ('cheby2', 1, (40.0,), 0.45, 'lowpass'), 9.991e-01),
    Cell(('zpn', 25, 4, 2, 5), 1400, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 25, 4, 2, 8), 129, 0.2, ('cheby1', 3, (3.0,), (0.05, 0.3), 'bandpass'), 3.239e-01),
    Cell(('zpn', 25, 4, 4, 5), 1400, 0.2, ('cheby1', 3, (3.0,), (0.2, 0.4), 'bandpass'), 4.890e-01),
    Cell(('zpn', 25, 4, 4, 8), 400, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.260e-01),
    Cell(('zpn', 25, 6, 2, 5), 1400, 0.2, ('cheby1', 9, (1.0,), 0.3, 'lowpass'), 2.571e-01),
    Cell(('zpn', 25, 6, 2, 8), 257, 0.2, ('ellip', 9, (1.0, 80.0), 0.45, 'lowpass'), 1.854e-01),
    Cell(('zpn', 25, 6, 4, 5), 1400, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandstop'), 3.001e-01),
    Cell(('zpn', 25, 6, 4, 8), 129, 0.2, ('cheby1', 10, (3.0,), 0.45, 'lowpass'), 2.827e-01),
    Cell(('zpn', 25, 6, 6, 5), 1400, 0.2, ('cheby2', 6, (80.0,), (0.2, 0.4), 'bandpass'), 2.766e-04),
    Cell(('zpn', 25, 6, 6, 8), 2, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandpass'), 4.049e-01),
    Cell(('zpn', 25, 8, 2, 5), 1400, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.990e-02),
    Cell(('zpn', 25, 8, 2, 8), 129, 0.2, ('cheby2', 15, (40.0,), 0.2, 'lowpass'), 4.931e-04),
    Cell(('zpn', 25, 8, 4, 5), 1400, 0.2, ('ellip', 7, (0.1, 70.0), (0.3, 0.6), 'bandstop'), 2.782e-02),   # (re-picked: lowest model error)
    Cell(('zpn', 25, 8, 4, 8), 300, 0.2, ('cheby1', 13, (1.0,), 0.45, 'lowpass'), 1.647e-01),
    Cell(('zpn', 25, 8, 6, 8), 513, 0.2, ('cheby1', 7, (0.1,), (0.2, 0.4), 'bandpass'), 1.880e-05),   # (re-picked: lowest model error)
    Cell(('zpn', 26, 2, 2, 5), 1100, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('zpn', 26, 2, 2, 8), 2, 0.2, ('cheby2', 1, (60.0,), 0.05, 'highpass'), 1.000e+00),
    Cell(('zpn', 26, 4, 2, 5), 1100, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 26, 4, 2, 8), 400, 0.2, ('cheby1', 3, (3.0,), (0.05, 0.3), 'bandpass'), 3.239e-01),
    Cell(('zpn', 26, 4, 4, 5), 1100, 0.2, ('cheby1', 3, (3.0,), (0.2, 0.4), 'bandpass'), 4.890e-01),
    Cell(('zpn', 26, 4, 4, 8), 900, 0.2, ('cheby1', 5, (3.0,), 0.1, 'lowpass'), 5.260e-01),
    Cell(('zpn', 26, 6, 2, 5), 1100, 0.2, ('cheby1', 9, (1.0,), 0.3, 'lowpass'), 2.571e-01),
    Cell(('zpn', 26, 6, 2, 8), 2, 0.2, ('cheby1', 9, (1.0,), 0.3, 'highpass'), 1.669e-01),
    Cell(('zpn', 26, 6, 4, 5), 1100, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandstop'), 3.001e-01),
    Cell(('zpn', 26, 6, 4, 8), 64, 0.2, ('cheby1', 9, (3.0,), 0.45, 'lowpass'), 3.516e-01),
    Cell(('zpn', 26, 6, 6, 5), 1100, 0.2, ('cheby2', 6, (80.0,), (0.2, 0.4), 'bandpass'), 2.766e-04),
    Cell(('zpn', 26, 6, 6, 8), 2, 0.2, ('cheby1', 6, (1.0,), (0.3, 0.6), 'bandpass'), 1.988e-01),
    Cell(('zpn', 26, 8, 2, 5), 1100, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.990e-02),
    Cell(('zpn', 26, 8, 2, 8), 2, 0.2, ('cheby2', 16, (40.0,), 0.3, 'lowpass'), 6.720e-04),
    Cell(('zpn', 26, 8, 4, 5), 1100, 0.2, ('ellip', 7, (0.1, 70.0), (0.3, 0.6), 'bandstop'), 2.782e-02),   # (re-picked: lowest model error)
    Cell(('zpn', 26, 8, 4, 8), 64, 0.2, ('cheby1', 7, (1.0,), (0.3, 0.6), 'bandstop'), 1.610e-01),
    Cell(('zpn', 26, 8, 6, 8), 2, 0.2, ('cheby1', 8, (0.1,), (0.3, 0.6), 'bandpass'), 7.210e-05),
    Cell(('zpn', 27, 2, 2, 5), 900, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('zpn', 27, 4, 2, 5), 900, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 27, 4, 4, 5), 900, 0.2, ('cheby1', 3, (3.0,), (0.2, 0.4), 'bandpass'), 4.890e-01),
    Cell(('zpn', 27, 6, 2, 5), 769, 0.2, ('cheby1', 9, (1.0,), 0.3, 'lowpass'), 2.571e-01),
    Cell(('zpn', 27, 6, 4, 5), 64, 0.2, ('cheby1', 5, (3.0,), (0.3, 0.6), 'bandstop'), 3.001e-01),
    Cell(('zpn', 27, 6, 6, 5), 2, 0.2, ('cheby2', 5, (80.0,), (0.15, 0.17), 'bandstop'), 7.484e-04),
    Cell(('zpn', 27, 8, 2, 5), 900, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.990e-02),
    Cell(('zpn', 27, 8, 4, 5), 2, 0.2, ('cheby1', 7, (0.1,), (0.3, 0.6), 'bandstop'), 4.125e-02),
    Cell(('zpn', 27, 8, 6, 5), 2, 0.2, ('cheby2', 7, (80.0,), (0.2, 0.4), 'bandpass'), 4.889e-07),
    Cell(('zpn', 28, 2, 2, 5), 2, 0.2, ('cheby1', 1, (1.0,), 0.025, 'highpass'), 1.000e+00),
    Cell(('zpn', 28, 4, 2, 5), 129, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 28, 4, 4, 5), 2, 0.2, ('cheby1', 5, (3.0,), 0.2, 'lowpass'), 5.457e-01),
    Cell(('zpn', 28, 6, 2, 5), 33, 0.2, ('cheby1', 9, (1.0,), 0.45, 'lowpass'), 2.328e-01),
    Cell(('zpn', 28, 6, 4, 5), 2, 0.2, ('cheby1', 5, (1.0,), (0.3, 0.6), 'bandpass'), 2.470e-01),
    Cell(('zpn', 28, 6, 6, 5), 513, 0.2, ('cheby2', 5, (80.0,), (0.15, 0.17), 'bandstop'), 7.484e-04),
    Cell(('zpn', 28, 8, 2, 5), 257, 0.2, ('cheby1', 13, (0.1,), 0.45, 'lowpass'), 4.990e-02),
    Cell(('zpn', 28, 8, 4, 5), 33, 0.2, ('cheby1', 7, (0.1,), (0.3, 0.6), 'bandstop'), 4.125e-02),
    Cell(('zpn', 29, 2, 2, 5), 2, 0.2, ('butter', 1, (), 0.015, 'lowpass'), 1.000e+00),
    Cell(('zpn', 29, 4, 2, 5), 2, 0.2, ('cheby1', 5, (3.0,), 0.3, 'lowpass'), 5.054e-01),
    Cell(('zpn', 29, 4, 4, 5), 2, 0.2, ('cheby2', 3, (80.0,), (0.3, 0.6), 'bandstop'), 2.553e-01),
    Cell(('zpn', 29, 6, 2, 5), 64, 0.2, ('cheby1', 5, (1.0,), (0.3, 0.6), 'bandstop'), 1.830e-01),
    Cell(('zpn', 29, 6, 4, 5), 33, 0.2, ('cheby2', 6, (80.0,), (0.3, 0.6), 'bandpass'), 4.361e-03),
    Cell(('zpn', 29, 8, 2, 5), 2, 0.2, ('cheby2', 7, (40.0,), (0.3, 0.6), 'bandstop'), 1.081e-02),
    Cell(('zpn', 29, 8, 4, 5), 257, 0.2, ('cheby2', 7, (40.0,), (0.2, 0.4), 'bandstop'), 2.821e-03),
    Cell(('zpn', 30, 2, 2, 5), 2, 0.2, ('butter', 1, (), 0.05, 'lowpass'), 1.000e+00),
    Cell(('zpn', 30, 4, 2, 5), 33, 0.2, ('cheby1', 5, (3.0,), 0.45, 'lowpass'), 4.587e-01),
    Cell(('zpn', 30, 6, 2, 5), 129, 0.2, ('cheby1', 9, (0.1,), 0.45, 'lowpass'), 7.661e-02),
    Cell(('zpn', 30, 8, 2, 5), 33, 0.2, ('cheby2', 7, (40.0,), (0.3, 0.6), 'bandstop'), 1.081e-02),
]


def _unreached():
    u = {}
    for nr in range(8, 16):
        for nm in (2, 4, 6):
            u[("zp", nr, nm)] = ("build_zpn accepts every pair build_zp accepts (its search tries NB = NR + 16 with the "
                                 "same guard rows D = 16 - NR, its fit floor 3e-7 lies under build_zp's 1e-3, both "
                                 "take at most six modes), so chain_zp.hip never falls back to the pair kernel")
    for nm in (2, 4, 6):
        u[("spec", 8, nm)] = "spec::build takes R <= 2 NR - 16 burst rows: none at NR = 8"
        u[("spec", 15, nm)] = "spec::build caps NR at (3841 - wlen) / 256, 14 for the shortest FIR (2 taps)"
    for nr in range(9, 15):
        for nm in (2, 4):
            u[("spec", nr, nm)] = ("the pair route needs build_specn to refuse and spec::build to accept; with four "
                                   "modes or fewer build_specn refused none of the sweep's designs that build took")
    for nb, nm in ((21, 8), (22, 8)):          # (and R + Rf <= 2 NB - 32, see below)
        u[("zpn", nb, nm, 2, 12)] = ("build_zpn picks NB <= 22 only for a left tail of R = 32 - NB >= 10 rows; "
                                     "no %d-mode design of the sweep with such a tail has just two slow modes" % nm)
    for nm, ns in ((2, 2), (4, 2), (4, 4), (6, 2), (6, 4), (6, 6), (8, 2), (8, 4), (8, 6)):
        u[("zpn", 20, nm, ns, 12)] = ("build_zpn keeps the held rows below the carried ones (R + Rf <= 2 NB - 32 = 8 at "
                                      "NB = 20), and a tail of at most eight rows fits a larger block unless its right "
                                      "tail rules blocks of 21 ... 23 out: no design of the sweep")
    for nm, ns in ((2, 2), (4, 2), (4, 4), (6, 2), (6, 4), (6, 6), (8, 4), (8, 6)):
        u[("zpn", 21, nm, ns, 12)] = ("build_zpn keeps the held rows below the carried ones (R + Rf <= 2 NB - 32 = 10 "
                                      "at NB = 21), and such tails fit a larger block unless its right tail rules "
                                      "blocks of 22 and 23 out: no design of the sweep")
    for nm, ns in ((2, 2), (6, 4)):
        u[("zpn", 22, nm, ns, 12)] = ("R + Rf <= 2 NB - 32 = 12 at NB = 22 (held rows below the carried ones): the "
                                      "sweep's designs for this class take other blocks or routes")
    for nb, nm, ns in ((30, 4, 4), (30, 6, 4), (30, 8, 4), (30, 6, 6), (30, 8, 6), (29, 6, 6), (29, 8, 6)):
        u[("zpn", nb, nm, ns, 5)] = ("NB = %d (wlen <= %d) leaves D = %d guard rows, so the left tail must end "
                                     "within %d rows while %d modes ring past 257 samples (NS = %d): no design of the "
                                     "sweep does both" % (nb, 7937 - 256 * nb, 32 - nb, 32 - nb, ns, ns))
    for nb in (24, 25, 26, 28):
        u[("zpn", nb, 8, 6, 5)] = ("eight modes of which exactly six slow (NS 6 < NM 8) with a left tail of at most "
                                   "five rows at NB = %d: no design of the sweep" % nb)
    return u


# compiled instances no (FIR, design) pair reaches, with the planner's reason
UNREACHED = _unreached()


def tolerance(c):
    """Per-cell error bound relative to a channel's max |reference| (the fit's error
    is about 1e-16 / ratio of the output scale; the stated worst case is 1e-9)."""
    return min(max(1e-11, 30e-16 / c.ratio), 1e-9)


def cell_id(c):
    return "-".join(str(v) for v in c.cell)


_NM_RE = {
    "zpn": re.compile(r"chain_zpn_kernel<(\d+), (\d+), (\d+), (\d+), true>"),
    "fwd": re.compile(r"chain_zpn_kernel<(\d+), (\d+), (\d+), 5, false>"),
    "zp": re.compile(r"chain_zp_kernel<(\d+), (\d+), true>"),
    "spec": re.compile(r"chain_spec_kernel<(\d+), (\d+), 16>"),
    "scan": re.compile(r"chain_kernel<(\d+), (true|false)>"),
}


def compiled_cells(lib_path):
    """The cells compiled into the library, from `nm -C`."""
    out = subprocess.check_output(["nm", "-C", lib_path], text=True)
    cells = set()
    for fam, rx in _NM_RE.items():
        for m in rx.finditer(out):
            v = m.groups()
            if fam == "scan":
                cells.add(("scan", int(v[0]), int(v[1] == "true")))
            else:
                cells.add((fam,) + tuple(int(a) for a in v))
    return cells


# -------------------------------------------------------------------------- GPU stream helpers
def whole_stream_reference(xh, h, sos):
    """Forward pass from sosfilt_zi * u[0], backward pass over everything (zero-extended)."""
    total = xh.shape[1]
    u = sps.oaconvolve(xh, h[None], axes=-1)[:, :total]
    zi = sps.sosfilt_zi(sos)[:, None, :] * u[:, :1][None]
    f, _ = sps.sosfilt(sos, u, axis=-1, zi=zi)
    ext = np.concatenate([f, np.zeros((xh.shape[0], 8192))], 1)
    return sps.sosfilt(sos, ext[:, ::-1], axis=-1)[:, ::-1][:, :total]


def run_stream(dev, x, h, sos, lens, split=False):
    """The chunks of x through osz_chain_zp_step; returns (outputs as one tensor whose
    column q is stream sample q - lag, lag).  split: the outputs of every step go to the
    tail of the previous chunk's buffer and the head of the current one, as a caller that
    cuts the stream into chunks of its own has them."""
    import torch
    C = x.shape[0]
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        lag = dev.chain_zp_lag(fir, iir)
        assert lag >= 0
        iir.set_state_scaled((x[:, :1] * float(h[0])).contiguous(), 0)
        dev.chain_zp_open(fir, iir, 0)
        outs, o = [], 0
        if not split:
            for n in lens:
                outs.append(dev.chain_zp_step(fir, iir, x[:, o:o + n]))
                o += n
            return torch.cat(outs, 1), lag
        cut = lag + 37                                        # where the caller's chunks begin
        bufs = [torch.full((C, cut), float("nan"), dtype=torch.float64, device="cuda")]
        for n in lens:
            bufs.append(torch.full((C, n), float("nan"), dtype=torch.float64, device="cuda"))
        for k, n in enumerate(lens):
            prev, cur = bufs[k], bufs[k + 1]
            dev.chain_zp_step(fir, iir, x[:, o:o + n], out=cur[:, :n - cut], tail=prev[:, prev.shape[1] - cut:])
            o += n
        return torch.cat([b[:, :b.shape[1]] for b in bufs], 1)[:, :sum(lens)], lag
    finally:
        fir.close()
        iir.close()
