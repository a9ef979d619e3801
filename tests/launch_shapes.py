"""The smallest batch at which every workgroup of an LDS-resident kernel runs past its first loop pass, from the text of
pffft_hip_describe() (tests/test_launch_shapes.py pins the arithmetic, tests/test_gpu_launch_shapes.py uses it).

The launchers (pffft_hip.hip launch_tiled / launch_stock / launch_c1024, one_tu.hip) start a grid of at most `CUs x per_cu` resident
workgroups (times K for the "K x resident set" Stockham routes, `groups / its` for the table routes) and let each of them loop over groups of
at most `vmax` vectors; up to `m` groups per workgroup they start one workgroup per group instead.  With

    B_long = (m + 3) x CUs x per_cu x vmax + r

every workgroup of the route's kernel therefore runs at least three groups beyond its launch rule's threshold, and r (odd, no multiple of
vmax) leaves the last pass ragged.  m is the printed oneshot of an in-order route and the table's groups per workgroup of a static-stride
table route (whose workgroups never run more than that many groups: the batch gives every one of them all of them).  For the
"K x resident set" routes K multiplies the GRID, it is no threshold: K + 3 resident sets of groups would give a workgroup 1 + 3 / K passes,
so there the factor is 3 K - three groups for every one of the K x CUs x per_cu workgroups, which is what `3 x grid x vmax <= B_long` asks
for.  Pure text and integer arithmetic: no device, no library."""
from __future__ import annotations

import re
from collections import namedtuple

LOOPING_KINDS = ("tiled", "c1024_f32", "stockham", "oneimage")
NO_LOOP_KINDS = ("tiny",)                 # one group per wavefront in dispatch order: nothing is reused from one vector to the next
LDS_PER_CU = 160 * 1024                   # gfx950: what the images of a CU's resident vectors share

LoopShape = namedtuple("LoopShape", "kind m vmax per_cu r B_long sets")


def route_body(line: str) -> str:
    """'  forward  ordered  : tiled: cfg ...' -> 'tiled: cfg ...' (a line without the (direction, layout) head is taken as it is)."""
    head, sep, body = line.strip().partition(": ")
    return body if sep and head.split()[0] in ("forward", "backward") else line.strip()


def core_vector_bytes(header: str) -> int:
    """Bytes of one core vector (n complex values of the setup's precision) from the first line of a describe() text."""
    m = re.search(r"pffft_hip setup N=\d+ (?:real|complex) (f32|f64): core n=(\d+),", header)
    if not m:
        raise ValueError(f"not the header line of a describe() text: {header!r}")
    return int(m.group(2)) * (16 if m.group(1) == "f64" else 8)


def ragged(vmax: int) -> int:
    """The smallest odd r >= 3 that is no multiple of vmax (vmax = 1: every r is one, 3 it is)."""
    r = 3
    while vmax > 1 and r % vmax == 0:
        r += 2
    return r


def _num(pattern: str, body: str) -> int:
    m = re.search(pattern, body)
    if not m:
        raise ValueError(f"the route line does not state {pattern!r}: {body!r}")
    return int(m.group(1))


def loop_shape(line: str, per_cu: int, cus: int, core_bytes: int = 0):
    """LoopShape of one route line (`per_cu`: pffft_hip_route_occupancy of the route, `cus`: the device's CU count, `core_bytes`:
    core_vector_bytes of the setup, read for Stockham plans only); None for a route that has no loop; ValueError for a line that is no
    LDS-resident route of a kind known here."""
    body = route_body(line)
    kind = body.split(":")[0]
    sets = None                                    # resident sets of full groups in the batch: m + 3 unless the route says otherwise
    if cus < 1:
        raise ValueError(f"CU count {cus}")
    if kind in NO_LOOP_KINDS:
        if "dispatch-order" not in body:
            raise ValueError(f"a {kind} route that is not in dispatch order: {body!r}")
        return None
    if kind == "c1024_f32":
        # the loop kernel runs past `m` resident sets of the short-launch kernel (the line states that set in wavefronts = vectors per CU)
        m = _num(r"<= (\d+) resident sets", body)
        vmax = _num(r"resident set (\d+) waves/CU", body)
        per_cu = _num(r"x (\d+) wg/CU", body)
        if "in-order" not in body:
            raise ValueError(f"unknown launch rule: {body!r}")
    elif kind == "tiled":
        if "in-order" not in body:
            raise ValueError(f"unknown launch rule: {body!r}")
        m = _num(r"oneshot<=(\d+) groups/wg", body)
        vmax = _num(r"vec/wg (\d+)", body)
    elif kind == "stockham":
        lds = _num(r" lds (\d+) ", body)
        if core_bytes < 1:
            raise ValueError("a Stockham plan needs the bytes of its core vector")
        vmax = max(1, lds // core_bytes)          # a workgroup's LDS holds the images of its vectors
        if "static-stride" in body:
            t = re.search(r"grid (\d+) groups/wg \(table\)", body)
            k = re.search(r"grid (\d+) x resident set", body)
            if not (t or k):
                raise ValueError(f"unknown static-stride grid: {body!r}")
            m = int((t or k).group(1))
            if k:
                sets = 3 * m
        elif "in-order grid resident set" in body:
            m = _num(r"oneshot<=(\d+) groups/wg", body) if "oneshot" in body else 0
        else:
            raise ValueError(f"unknown launch rule: {body!r}")
    elif kind == "oneimage":
        if "in-order" not in body or "per vector" not in body:
            raise ValueError(f"unknown launch rule: {body!r}")
        m, vmax = 0, 1
    else:
        raise ValueError(f"no LDS-resident route of a known kind: {body!r}")
    if per_cu < 1 or vmax < 1 or m < 0:
        raise ValueError(f"occupancy {per_cu}, vmax {vmax}, m {m}: {body!r}")
    r = ragged(vmax)
    sets = m + 3 if sets is None else sets
    return LoopShape(kind, m, vmax, per_cu, r, sets * cus * per_cu * vmax + r, sets)


def fused_long_batch(cus: int, core_bytes: int, m: int = 4) -> int:
    """The long batch of the fused kernels that follow the launch rule `groups <= m x grid` of the convolution kernel: a resident vector owns
    an LDS image of at least its own bytes, so floor(LDS / core vector bytes) bounds the vectors a CU's resident workgroups hold."""
    if cus < 1 or core_bytes < 1 or core_bytes > LDS_PER_CU:
        raise ValueError(f"CU count {cus}, core vector of {core_bytes} bytes")
    return (m + 3) * cus * (LDS_PER_CU // core_bytes) + 3


def sample_rows(batch: int, vmax: int, rng, random_rows: int = 64):
    """Sorted row numbers held to truth: the first 8, the last vmax + 3 and `random_rows` drawn from `rng` (numpy Generator)."""
    rows = set(range(min(8, batch))) | set(range(max(0, batch - (vmax + 3)), batch))
    rows |= set(int(v) for v in rng.integers(0, batch, random_rows))
    return sorted(rows)
