"""CPU tests (-m "not gpu") of the two kits the test files share.  tests/gpu_kit.py: kinds_by, by which every GPU test file reads a kineto
trace (the first matching substring of the table wins, a name that matches none is "other", the labels come in the order of the names);
the order in which alternating times its functions; what assert_refusal takes for a refusal.  tests/abi_kit.py: refused holds code AND
text, and the stand-in tensor answers what it was given and hands out no pointer."""
import pytest

import abi_kit
import gpu_kit as kit

TABLE = (("AnyRealIO", "real"), ("AnyChirpIO", "chirp"), ("any_real_pad_kernel", "pad"), ("fft_conv_kernel", "conv"))


def test_first_match_wins():
    assert kit.kinds_by(TABLE, ["void pf::fft_conv_kernel<AnyRealIO, AnyChirpIO>(...)"]) == ["real"]
    assert kit.kinds_by(TABLE, ["void pf::fft_conv_kernel<AnyChirpIO>(...)"]) == ["chirp"]
    assert kit.kinds_by(tuple(reversed(TABLE)), ["void pf::fft_conv_kernel<AnyRealIO, AnyChirpIO>(...)"]) == ["conv"]


def test_fallback_and_order():
    names = ["pf::any_real_pad_kernel", "stockham", "fft_conv_kernel<DenseIO>", "", "pf::any_real_pad_kernel"]
    assert kit.kinds_by(TABLE, names) == ["pad", "other", "conv", "other", "pad"]
    assert kit.kinds_by(TABLE, []) == [] and kit.kinds_by((), ["x"]) == ["other"]


def test_alternating_times_the_functions_in_their_order(monkeypatch):
    seen = []
    monkeypatch.setattr(kit, "best_of", lambda f: seen.append(f) or float(len(seen)))
    fns = tuple(lambda: None for _ in range(3))
    ts = kit.alternating(fns, rounds=2)
    assert seen == list(fns) * 2                                   # f0 f1 f2 f0 f1 f2
    assert ts == [[1.0, 4.0], [2.0, 5.0], [3.0, 6.0]]


def test_assert_refusal():
    msg = "pffft_hip: fft2: cannot grow the scratch during graph capture: hipErrorStreamCaptureUnsupported (900)"
    kit.assert_refusal(msg)
    kit.assert_refusal(msg, "(900)")
    kit.assert_refusal(msg + "; the tables of this setup", "(900)", "tables of this setup")
    with pytest.raises(AssertionError):
        kit.assert_refusal("")                                     # what a call that was NOT refused leaves behind
    with pytest.raises(AssertionError):
        kit.assert_refusal("", "(900)")
    with pytest.raises(AssertionError):
        kit.assert_refusal("refused during graph capture", "(900)")
    with pytest.raises(AssertionError):
        kit.assert_refusal("hipErrorStreamCaptureUnsupported (900)", "(900)")


def test_refused_holds_code_and_text(monkeypatch):
    monkeypatch.setattr(abi_kit.pa, "last_error", lambda: "pffft_hip: fft2: unknown direction")
    abi_kit.refused(1, abi_kit.INVALID_VALUE, "pffft_hip: fft2: unknown direction")
    with pytest.raises(AssertionError):
        abi_kit.refused(1, abi_kit.INVALID_VALUE, "pffft_hip: fft2: unknown directions")     # the code matches, one character more
    with pytest.raises(AssertionError):
        abi_kit.refused(400, abi_kit.INVALID_VALUE, "pffft_hip: fft2: unknown direction")    # the text matches, another code
    assert (abi_kit.INVALID_VALUE, abi_kit.INVALID_HANDLE) == (1, 400)
    assert (abi_kit.prefix(float), abi_kit.prefix("float32")) == ("pffftd", "pffft")


def test_fake_tensor():
    t = abi_kit.Fake(1536, "a dtype")
    assert (t.numel(), t.is_contiguous(), t.dtype, t.is_cuda) == (1536, True, "a dtype", True)
    assert abi_kit.Fake(0, None).numel() == 0
    with pytest.raises(AssertionError, match="a refused call reads no pointer"):
        t.data_ptr()
