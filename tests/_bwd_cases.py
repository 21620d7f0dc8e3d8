"""Inputs and launch geometry of the backward tests, shared by the CPU part (tests/test_backward_cases.py: the conditions the
inputs must meet) and the GPU part (tests/test_gpu_backward.py: the kernels against oracle.fakequant_oracle's float64 sums).

Geometry mirrored here from csrc/fq_backward.hip, csrc/fq_bodies.h and csrc/rootq.hip: workgroups of 256 lanes, one float4 per
lane and chunk (1024 elements), a per-tensor grid capped at 8192 workgroups, a 0-3 element tail owned by workgroup 0, a
per-channel plan of ceil(2048 / channels) segments (at most `outer`) of `npseg` rows, a RootQ grid capped at 1024 workgroups.
The per-channel plan's cap of 65 535 segments cannot be reached (nseg <= ceil(2048 / 2) = 1024), so nothing here tries."""
import functools
import math

import torch

from oracle import fakequant_oracle as O

BLOCK, CHUNK, TENSOR_BLOCKS, CUS8, RQ_BLOCKS = 256, 1024, 8192, 2048, 1024
MULTI_MAX_N = CHUNK * TENSOR_BLOCKS
BIG = MULTI_MAX_N + 2051                 # workgroups 0 and 1 take a second chunk, workgroup 0 a tail of 3
FORMS = ("qbase", "zeropoint", "symmetric", "rootq_act")
RANGE = {"qbase": (-8, 7), "zeropoint": (0, 15), "symmetric": (-7, 7), "rootq_act": (0, 15)}
UNIT = 2.0 ** -2                         # every contribution of an exact case is a multiple of it

# (outer, channels, inner): [forms]
TENSOR_N = (1, 3, 1023, 1024, 1025, 1027, 4099, 262148, MULTI_MAX_N)
TENSOR_SHAPES = [((1, 1, n), FORMS) for n in TENSOR_N] + [((1, 1, BIG), FORMS[:2])]
UNALIGNED_N = ((4099, FORMS), (BIG, FORMS[:2]))
# shape: (nseg, npseg) the plan must give - the geometry each shape is here for
CHANNEL_PLANS = {(5, 3, 7): (5, 1), (5, 1024, 12): (2, 3), (5, 1024, 9): (2, 3), (7, 700, 4): (3, 3), (3, 2049, 4): (1, 3),
                 (1, 257, 1028): (1, 1), (1, 257, 1027): (1, 1), (2, 64, 16): (2, 1)}
CHANNEL_FORMS = FORMS[:3]
MISALIGNED_CHANNEL_SHAPE = (2, 64, 16)   # inner % 4 == 0, sent through a view one float into its buffer: the generic kernel


def cdiv(a, b):
    return -(-a // b)


def plan(outer, ch, inner):
    """(nseg, npseg, grid_x) of csrc/fq_backward.hip `bwd_plan`; nseg * ch floats of scratch."""
    if ch == 1:
        b = min(max(cdiv((outer * inner) >> 2, BLOCK), 1), TENSOR_BLOCKS)
        return b, 0, b
    nseg = max(min(cdiv(CUS8, ch), outer), 1)
    npseg = cdiv(outer, nseg)
    return cdiv(outer, npseg), npseg, ch


def chain_length(outer, ch, inner, vec):
    """L: the longest chain of additions one lane performs before the workgroup's tree - passes per lane times 4 on the float4
    path (the four contributions of a float4 and the accumulator), times 1 on the generic path, plus the tail element."""
    nseg, npseg, grid = plan(outer, ch, inner)
    if ch == 1:
        n = outer * inner
        if vec:
            return max(4 * cdiv(cdiv(n >> 2, BLOCK), grid) + (1 if n & 3 else 0), 1)
        return cdiv(n, grid * BLOCK)
    return max(npseg * (4 * cdiv(inner >> 2, BLOCK) if vec else cdiv(inner, BLOCK)), 1)


def sum_bound(L, abs_sum, g=1.0):
    """|fp32 tree sum - exact sum| <= (L + 13) * 2^-24 * sum|contrib| * g: each addition of a chain of depth D contributes a
    relative 2^-24 of the running sum's magnitude, at most sum|contrib|; D = L per lane, + 2 in the quad, + 6 across the wave,
    + 3 across the workgroup's four waves (the partials are then folded in float64), + 1 for the cast to fp32 and + 1 for the
    multiplication by g.  Underflow is not modelled (a product in the denormal range errs by up to 2^-150 whatever its size),
    so the random cases keep sum|contrib| far above that: tests/test_backward_cases.py asserts it."""
    return (L + 13) * 2.0 ** -24 * abs_sum * g


def adversarial(scale, offset, lo, hi):
    """tests/test_gpu_fq_multi.py `adversarial`, finite values only (a NaN or an infinity in x makes the whole sum NaN)."""
    from test_gpu_fq_multi import adversarial as adv
    a = adv(scale, offset, lo, hi)
    return a[torch.isfinite(a)]


# ------------------------------------------------------------------------------------------------------ edges
def planted_positions(outer, ch, inner):
    """Flat indices [P, ch] (one column per channel, whose sums are separate) of the elements on the launch geometry's edges.
    Per tensor: first and last element, both sides of chunk boundaries, every tail element.  At most 20 distinct powers of two
    fit under the 2^24 limit of an exact fp32 sum, so a tensor that crosses more than four boundaries gets them where the
    geometry changes: the first, those next to partial 256 (the finalize's stride), those at the grid cap and the last.
    Per channel: on the first and last row of every segment, the row's first element, the first and last element of its last
    float4, its last scalar, and both sides of a workgroup pass (256 scalars, 256 float4)."""
    if ch == 1:
        n = outer * inner
        last_k = (n - 1) // CHUNK
        ks = [k for k in (1, 2, 3, 4, 255, 256, TENSOR_BLOCKS - 1, TENSOR_BLOCKS, TENSOR_BLOCKS + 1, last_k) if 1 <= k <= last_k]
        if last_k > 4:
            ks = [k for k in ks if k not in (2, 3, 4)]
        idx = {0, n - 1} | {k * CHUNK - 1 for k in ks} | {k * CHUNK for k in ks} | set(range(n - (n & 3), n))
        return torch.tensor(sorted(idx), dtype=torch.int64).reshape(-1, 1)
    nseg, npseg, _ = plan(outer, ch, inner)
    rows = sorted({r for s in range(nseg) for r in (s * npseg, min((s + 1) * npseg, outer) - 1)})
    pos = {0, inner - 1} | {p for p in (BLOCK - 1, BLOCK, CHUNK - 1, CHUNK) if p < inner}
    if inner >= 4:
        pos |= {4 * (inner // 4) - 4, 4 * (inner // 4) - 1}
    c = torch.arange(ch, dtype=torch.int64)
    return torch.stack([(r * ch + c) * inner + p for r in rows for p in sorted(pos)])


class Case:
    """x, gy [outer, ch, inner]; scale, offset [ch]; planted: flat indices [P, ch] (exact cases)."""

    def __init__(self, kind, form, shape, x, gy, scale, offset, g, planted=None):
        self.kind, self.form, self.shape, self.x, self.gy, self.scale, self.offset, self.g = kind, form, shape, x, gy, scale, offset, g
        self.lo, self.hi = RANGE[form]
        self.planted = planted

    def reference(self):
        return O.fq_backward_f64(self.form, self.x, self.gy, self.scale, self.offset, self.lo, self.hi, self.g)


def exact_case(form, shape, seed=2333):
    """Dyadic inputs: scale 2^-4, dyadic offsets, x on multiples of 2^-6, gy in {-1, 0, 1} - every contribution a multiple of
    2^-2 - and gy = +-2^j (a distinct j per edge of a channel's sum) planted where v = k - 1/4, contribution +-2^(j-2)."""
    outer, ch, inner = shape
    n = outer * ch * inner
    lo, hi = RANGE[form]
    gen = torch.Generator().manual_seed(seed)
    s = 2.0 ** -4
    c = torch.arange(ch)
    off = {"qbase": ((c % 5) - 2).float() * 2.0 ** -3, "zeropoint": (c % 4 + 1).float()}.get(form)
    zp = off.reshape(1, ch, 1) if form == "zeropoint" else torch.zeros(1, 1, 1)
    span = hi - lo
    vlo = (lo - zp) if form != "rootq_act" else torch.zeros(1, 1, 1)         # the lowest in-range v, per channel
    v = torch.randint(1, span, shape, generator=gen).float() + vlo            # on the grid, strictly inside
    gy = torch.randint(-1, 2, shape, generator=gen).float()
    flat = torch.arange(n).reshape(shape)
    live = flat % 16 == 5                                                      # off the grid by 1/4, 1/2 (a tie) or 3/4
    v = torch.where(live, v + torch.randint(1, 4, shape, generator=gen).float() / 4, v)      # still below the top code
    step = 0.25 if form in ("qbase", "rootq_act") else 0.75                    # the first step whose code leaves the range
    v = torch.where(flat % 128 == 77, vlo + span + step, v)
    v = torch.where(flat % 128 == 13, vlo - step, v)
    planted = planted_positions(*shape)
    assert planted.shape[0] <= 20, "more planted powers of two than an exact fp32 sum holds"
    vf, gf = v.reshape(-1), gy.reshape(-1)
    vlo_f = vlo.expand(shape).reshape(-1)
    for j in range(planted.shape[0]):
        vf[planted[j]] = vlo_f[planted[j]] + 1 + (j % 3) - 0.25
        gf[planted[j]] = (-1.0) ** j * 2.0 ** j
    x = v * s + (off.reshape(1, ch, 1) if form == "qbase" else 0.0)
    assert torch.equal(x, (x * 64).round() / 64), "x must lie on multiples of 2^-6"
    return Case("exact", form, shape, x.contiguous(), gy, torch.full((ch,), s), off, 2.0 ** -10 if form == "qbase" else 0.0, planted)


def random_case(form, shape, seed=4242):
    """Random x, gy (one in 13 zero) and scales, with the quantiser's ties and clamp edges (one ulp either side, both zeros,
    denormals) of channel 0 at the head of the tensor."""
    outer, ch, inner = shape
    lo, hi = RANGE[form]
    gen = torch.Generator().manual_seed(seed + 7 * FORMS.index(form))
    scale = torch.rand(ch, generator=gen) * 0.05 + 0.01
    scale[0] = 2.0 ** -4
    off = {"qbase": torch.randn(ch, generator=gen) * 0.05 + 0.0137,
           "zeropoint": torch.randint(lo + 1, hi, (ch,), generator=gen).float()}.get(form)
    x = torch.randn(shape, generator=gen) * 0.4 + (0.3 if form == "rootq_act" else 0.0)
    adv = adversarial(float(scale[0]), float(off[0]) if form == "qbase" else 0.0, lo, hi)
    if outer * inner >= 16:            # (a sum of nothing but denormal products is outside the bound's model: see sum_bound)
        m = min(adv.numel(), inner)
        x[0, 0, :m] = adv[:m]
    gy = torch.randn(shape, generator=gen)
    gy.view(-1)[::13] = 0.0
    g = 1 / math.sqrt(outer * ch * inner * hi) if form == "qbase" else 0.0
    return Case("random", form, shape, x, gy, scale, off, g)


@functools.lru_cache(maxsize=2)
def case_with_reference(kind, form, shape):
    """The case and (gx, value, abs_sum, contrib) - computed once for all tests that launch it (they run next to each other)."""
    case = (exact_case if kind == "exact" else random_case)(form, shape)
    return case, case.reference()


def all_fq_cases():
    """(form, shape) of every fake-quant geometry."""
    out = [(f, shape) for shape, forms in TENSOR_SHAPES for f in forms]
    return out + [(f, shape) for shape in CHANNEL_PLANS for f in CHANNEL_FORMS]


# ------------------------------------------------------------------------------------------------------ RootQ weights
RQ_N = (1, 255, 257, 65537, 262144, 262144 + 257)
RQ_BITS = (4, 2)
RQ_ALPHA = (0.25, 1.5)
RQ_PLANT_GY = 2.0 ** 12
RQ_INDICES = (0, -1, 262143, 262144, 262400)       # -1: n - 1


class RootqCase:
    def __init__(self, n, bits, alpha, seed=99):
        self.n, self.bits, self.alpha = n, bits, alpha
        self.hi = 2 ** (bits - 1) - 1
        self.lo = -self.hi
        gen = torch.Generator().manual_seed(seed + n % 1000 + bits)
        self.w = torch.randn(n, generator=gen) * 0.1
        # small everywhere else, so that one planted element outweighs the tolerance of the whole sum
        self.gy = torch.randn(n, generator=gen) * 2.0 ** -7
        self.upper = 0.16 * math.sqrt(self.hi)
        self.lower = -self.upper
        delta = (self.upper - self.lower) / (self.hi - self.lo)
        # the listed indices: inside the first interval, just above its middle, where B = k|e| + 1e-5 is far from 1 and the
        # element moves g_alpha as well as g_lower;  two more, next to the ends, clipped above: they move g_upper
        self.planted = sorted({i % n for i in RQ_INDICES if -n <= i < n})
        self.planted_above = sorted({i for i in (1, n - 2) if 0 <= i < n and i not in self.planted}) if n >= 4 else []
        for j, i in enumerate(self.planted):
            self.w[i] = self.lower + (0.5 + 0.01) * delta
            self.gy[i] = RQ_PLANT_GY * (-1.0) ** j
        for j, i in enumerate(self.planted_above):
            self.w[i] = self.upper + 0.05
            self.gy[i] = RQ_PLANT_GY * (-1.0) ** j
        self.passes = cdiv(n, min(cdiv(n, BLOCK), RQ_BLOCKS) * BLOCK)
        self.L = 2 * self.passes           # the kernel's longest chain: two `+=` per element on the d and l sums

    def reference(self, gy=None):
        return O.rootq_weight_backward_f64(self.w, self.gy if gy is None else gy, self.upper, self.lower, self.alpha, self.lo, self.hi)

    def bounds(self, abs_sums):
        """Tolerance of (g_upper, g_lower, g_alpha): the project's elementwise 2e-4 carried through the sum, plus the summation
        bound, over the addends that feed each scalar."""
        r = self.hi - self.lo
        feed = (abs_sums["u"] + abs_sums["d"] / r, abs_sums["l"] + abs_sums["d"] / r, abs_sums["a"])
        return tuple(float(2e-4 * f + sum_bound(self.L, f)) for f in feed)


@functools.lru_cache(maxsize=4)
def rootq_case(n, bits, alpha):
    case = RootqCase(n, bits, alpha)
    return case, case.reference()
