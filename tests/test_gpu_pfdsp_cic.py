"""GPU tests (-m gpu) of the PFDSP CIC down-converter and carriers on MI355X (libpfdsp_hip.so; kernels in
pffft_amd/csrc/pfdsp_cic.h).  Every comparison is bit for bit: against the reference's own outputs recorded in
tests/golden/pfdsp_cic_golden.npz and against the numpy restatement tests/cic_model.py."""
import ctypes as C
import os

import numpy as np
import pytest

import cic_model as cm
from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from pffft_amd import pfdsp  # noqa: E402

W = {"s16": 1, "cs16": 2, "cu8": 2}
NP_DT = {"s16": np.int16, "cs16": np.int16, "cu8": np.uint8}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device: the product has no CPU fallback")
    torch.cuda.set_device(0)
    pfdsp.cic_lib()


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "pfdsp_cic_golden.npz")))


def same(a, b):
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _input(fmt, n_out, R, seed):
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if fmt == "cu8" else (-32768, 32768)
    return rng.integers(lo, hi, n_out * R * W[fmt], dtype=NP_DT[fmt])


def _model(fmt, R, x, calls):
    """outputs of the model over consecutive calls [(outsize, rate), ...] on one state"""
    st, pos, ys = cm.State(R), 0, []
    for n, r in calls:
        ys.append(cm.run(st, fmt, x[pos:pos + n * R * W[fmt]], n, r))
        pos += n * R * W[fmt]
    return np.concatenate(ys)


@pytest.mark.parametrize("where", ["host", "device"])
def test_legacy_entries_against_reference(G, where):
    """cicddc_{s16,cs16,cu8}_c on host pointers (staged) and device pointers: the reference's recorded chains of every
    format and factor, saturating rates, outsize 1 and 2 inside the chain, extreme inputs"""
    errs = pfdsp.cic_lib().dll.pfdsp_hip_cic_error_count()
    n = 0
    for k in sorted(G):
        if not k.endswith("_y"):
            continue
        base = k[:-2]
        fmt, R = base.split("_")[1], int(base.split("_")[2])
        x, d, pos, got = G[base + "_x"], pfdsp.CicDdc(R), 0, []
        for m, r in zip(G[base + "_outsizes"], G[base + "_rates"]):
            seg = np.ascontiguousarray(x[pos:pos + int(m) * R * W[fmt]])
            pos += seg.size
            if where == "device":
                got.append(getattr(d, fmt)(torch.from_numpy(seg).cuda(), int(m), float(r)).cpu().numpy())
            else:
                got.append(getattr(d, fmt)(seg, int(m), float(r)))
        d.close()
        assert same(np.concatenate(got), G[k]), (base, where)
        n += 1
    assert n == 18
    assert pfdsp.cic_lib().dll.pfdsp_hip_cic_error_count() == errs


SPLITS = ([1] * 5 + [2] * 3, [2, 1, 1], [7, 1, 2, 33], [1, 2], [3])


@pytest.mark.parametrize("fmt", cm.FORMATS)
@pytest.mark.parametrize("R", [1, 3, 64, 1000])
def test_split_calls_equal_one_call(fmt, R):
    """one call of K outputs == the same input in any sequence of calls (outsize 1 and 2, boundaries right after the
    first one or two outputs of a call, where the incoming state enters) == the model"""
    K = 60 if R == 1000 else 700
    x = _input(fmt, K, R, 1000 + R)
    xd = torch.from_numpy(x).cuda()
    one = pfdsp.CicDdc(R)
    y1 = getattr(one, fmt)(xd, K, 0.137).cpu().numpy()
    assert same(y1, _model(fmt, R, x, [(K, 0.137)]))
    for split in SPLITS:
        sizes = split + [K - sum(split)]
        d, pos, parts = pfdsp.CicDdc(R), 0, []
        for n in sizes:
            parts.append(getattr(d, fmt)(xd[pos * R * W[fmt]:(pos + n) * R * W[fmt]], n, 0.137).cpu().numpy())
            pos += n
        assert same(np.concatenate(parts), y1), (fmt, R, split)


@pytest.mark.parametrize("R", [1, 2, 8, 64, 1000])
def test_large_call_against_model(R):
    """2^26 input samples in one call (every workgroup boundary of a full grid), then a short call on the state it left"""
    fmt = "cs16"
    K = (1 << 26) // R
    x = _input(fmt, K + 5, R, R)
    xd = torch.from_numpy(x).cuda()
    d = pfdsp.CicDdc(R)
    y = d.cs16(xd[:K * R * 2], K, 0.0123).cpu().numpy()
    y2 = d.cs16(xd[K * R * 2:], 5, -0.31).cpu().numpy()
    st, step = cm.State(R), max(1, (1 << 21) // R)
    for k0 in range(0, K, step):
        n = min(step, K - k0)
        assert same(y[k0:k0 + n], cm.run(st, fmt, x[k0 * R * 2:(k0 + n) * R * 2], n, 0.0123)), (R, k0)
    assert same(y2, cm.run(st, fmt, x[K * R * 2:], 5, -0.31)), R


def test_device_entry_on_a_stream_chained_without_syncs():
    R = 16
    calls = [(1, 0.2), (3000, -0.45), (2, 0.2), (777, 0.0071)]
    x = _input("cu8", sum(n for n, _ in calls), R, 5)
    xd = torch.from_numpy(x).cuda()
    d = pfdsp.CicDdc(R)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs, pos = [], 0
    with torch.cuda.stream(s):
        for n, r in calls:
            outs.append(pfdsp.cicddc_bank([d], [r], "cu8", xd[pos * R * 2:(pos + n) * R * 2], n))
            pos += n
    s.synchronize()
    assert same(torch.cat([o[0] for o in outs]).cpu().numpy(), _model("cu8", R, x, calls))


def test_graph_replay_advances_the_state():
    """two chained calls captured once and replayed twice == four plain calls"""
    R, K, rate = 8, 4096, 0.05
    x = _input("cs16", K, R, 9)
    xd = torch.from_numpy(x).cuda()
    plain = pfdsp.CicDdc(R)
    want = [pfdsp.cicddc_bank([plain], [rate], "cs16", xd, K).cpu().numpy() for _ in range(4)]
    st = cm.State(R)
    for w in want:
        assert same(w[0], cm.run(st, "cs16", x, K, rate))
    d = pfdsp.CicDdc(R)
    pfdsp.cicddc_bank([d], [rate], "cs16", xd, 0)          # binds the state before the capture
    o1 = torch.empty((1, K), dtype=torch.complex64, device="cuda")
    o2 = torch.empty((1, K), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pfdsp.cicddc_bank([d], [rate], "cs16", xd, K, out=o1)
        pfdsp.cicddc_bank([d], [rate], "cs16", xd, K, out=o2)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert same(o1.cpu().numpy(), want[2 * rep]) and same(o2.cpu().numpy(), want[2 * rep + 1]), rep


@pytest.mark.parametrize("nch", [1, 3, 64, 130])
def test_bank_equals_per_channel_calls(nch):
    """nch states with their own rates over one input, out_stride > outsize, two chained bank calls == per channel:
    the model, and the legacy entry on each channel's own state; nothing written between the rows"""
    R, calls = 32, [(777, None), (100, None)]
    rates = np.linspace(-0.45, 0.7, nch).astype(np.float32)
    x = _input("cs16", sum(n for n, _ in calls), R, nch)
    xd = torch.from_numpy(x).cuda()
    bank = [pfdsp.CicDdc(R) for _ in range(nch)]
    got, pos = [], 0
    for n, _ in calls:
        stride = n + 13
        buf = torch.full((nch, stride), float("nan"), dtype=torch.complex64, device="cuda")
        pfdsp.cicddc_bank(bank, rates, "cs16", xd[pos * R * 2:(pos + n) * R * 2], n, out=buf[:, :n])
        pos += n
        h = buf.cpu().numpy()
        assert np.all(np.isnan(h[:, n:].real)), nch
        got.append(h[:, :n])
    got = np.concatenate(got, axis=1)
    for c in range(0, nch, max(1, nch // 8)):
        assert same(got[c], _model("cs16", R, x, [(n, float(rates[c])) for n, _ in calls])), (nch, c)
    if nch <= 3:
        for c in range(nch):
            d, pos, parts = pfdsp.CicDdc(R), 0, []
            for n, _ in calls:
                parts.append(d.cs16(xd[pos * R * 2:(pos + n) * R * 2], n, float(rates[c])).cpu().numpy())
                pos += n
            assert same(np.concatenate(parts), got[c])


def test_invalid_arguments_return_errors_and_write_nothing():
    L = pfdsp.cic_lib().dll
    a, b, c16 = pfdsp.CicDdc(8), pfdsp.CicDdc(8), pfdsp.CicDdc(16)
    K = 10
    x = _input("cs16", K, 16, 3)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((2, 16), float("nan"), dtype=torch.complex64, device="cuda")

    def call(states, nch=None, fmt=1, xp=None, k=K, stride=16, rates=(0.1, 0.2)):
        nch = len(states) if nch is None else nch
        hs = (C.c_void_p * max(len(states), 1))(*[s.handle if s is not None else None for s in states])
        rs = (C.c_float * 2)(*rates)
        return L.pfdsp_hip_cicddc_device(hs, rs, nch, fmt, xp if xp is not None else xd.data_ptr(), k, out.data_ptr(),
                                         stride, None)

    assert call([a, None]) != 0
    assert call([a, a]) != 0
    assert call([a, c16]) != 0
    assert call([a, b], stride=9) != 0
    assert call([a, b], fmt=3) != 0 and call([a, b], fmt=-1) != 0
    assert call([a, b], nch=0) != 0
    assert L.pfdsp_hip_cicddc_device(None, None, 1, 1, xd.data_ptr(), K, out.data_ptr(), 16, None) != 0
    assert call([a, b], xp=0) != 0                           # NULL input with outsize > 0
    torch.cuda.synchronize()
    assert torch.isnan(out.real).all()
    assert L.pfdsp_hip_cic_last_error()
    # the states are unchanged: a valid call now equals a fresh state's
    y = pfdsp.cicddc_bank([a], [0.1], "cs16", xd, K).cpu().numpy()
    assert same(y[0], _model("cs16", 8, x, [(K, 0.1)]))


@pytest.mark.parametrize("name", pfdsp.CARRIERS)
def test_carriers_on_device_pointers(G, name):
    tdt = torch.float32 if name.endswith("_f") else torch.int16
    for size in (4, 12, 64, 6, 1, 1000003):
        n = 2 * size
        out = torch.full((n + 40,), 5, dtype=tdt, device="cuda")
        pfdsp.generate(name, size, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], cm.carrier(name, size)), (name, size)
        assert np.all(got[n:] == 5), (name, size)
        if size in (4, 12, 64):
            assert np.array_equal(got[:n], G[f"carrier_{name}_{size}"])
