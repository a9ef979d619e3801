"""CPU test (-m "not gpu") of tests/gpu_kit.py's kinds_by, by which every GPU test file reads a kineto trace: the first matching substring
of the table wins, a name that matches none is "other", and the labels come in the order of the names."""
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
