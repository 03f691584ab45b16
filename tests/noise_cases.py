"""Fixed inputs, floors and bars shared by tests/test_noise_ref_cpu.py and
tests/test_actor_noise_keyed_gpu.py (the keyed comparison of the fp32 actor's
exploration noise with oracle/noise_ref.py).

Everything here runs on the CPU: the nets are built by torch's CPU generator,
the inputs by numpy, and every floor is the restatement evaluated in fp32
against itself in fp64 -- never against a kernel.

Bars (nothing hard-coded):
  E_exact[sd], E_bf16[sd]  max |fp32 run - fp64 run| of the noisy forward with
                           exact / bf16 squares over both nets, both
                           (seed, counter) pairs, both calls, action_sd in
                           {0, ACTION_SD}
  E_z                      the same on the action-noise normals alone
  E_clean                  the same at sd = 0 (no noise)
  bar = FACTOR x floor (FACTOR = 16: room for the hardware log / sin / cos and
        the MFMA's summation order; supposed, not measured)
  cap[sd] = 1/4 of the smallest max-deviation of the mutant with sd x 1.01
        over the same cases; cap_z the same for action_sd x 1.01 on z
  bar_clean = CLEAN_FACTOR x E_clean, held below 0.8 x the smallest deviation
        of the split GEMM with one class of piece products dropped
"""
import functools

import numpy as np

from oracle import keras_ref, noise_ref

ROWS = 67
ROW_COUNTS = (1, 5, 67)
SDS = (0.1, 0.5)
ACTION_SD = 0.15
# (seed, device counter before the first call): the second pair's first call
# number is 2^32, so the high words of both seed and call count
SEED_CASES = ((5, 0), (0x0123456789ABCDEF, 2 ** 32 - 1))
NETS = ("default", "biased")
FACTOR = 16
CLEAN_FACTOR = 3
# the piece-product classes whose loss the noise-free bar must see
DROPPED = {"x_lo.w_hi": (2, 0), "x_hi.w_lo": (0, 2), "x_mid.w_mid": (1, 1)}


@functools.lru_cache(maxsize=None)
def actor(name):
    """torch Actor on the CPU: 'default' = seeded default init (unsaturated),
    'biased' = another seed with biases N(0, 0.1), so b^2 carries weight in
    the variance"""
    import torch

    from skillshot_learning_amd import learner
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed({"default": 101, "biased": 202}[name])
        a = learner.Actor()
        if name == "biased":
            with torch.no_grad():
                for l in (a.l1, a.l2, a.l3):
                    l.bias.normal_(0, 0.1)
    finally:
        torch.random.set_rng_state(state)
    return a


@functools.lru_cache(maxsize=None)
def params(name):
    return keras_ref.from_module(actor(name))


@functools.lru_cache(maxsize=None)
def inputs():
    """fp32 [ROWS, 12] observation-like rows: nonnegative, columns 4 and 9 up
    to 9.85, columns 5 and 11 mostly 0, some entries exactly 0 and exactly 1"""
    r = np.random.RandomState(20)
    x = r.rand(ROWS, 12)
    x[:, [4, 9]] *= 9.85
    x[:, [5, 11]] *= r.rand(ROWS, 2) < 0.3
    unit = [c for c in range(12) if c not in (4, 9)]
    pick = r.rand(ROWS, len(unit))
    xu = x[:, unit]
    xu[pick < 0.06] = 0.0
    xu[pick > 0.94] = 1.0
    x[:, unit] = xu
    x[3, 4], x[7, 9] = 9.85, 0.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def calls(counter0):
    """the two consecutive call numbers of a kernel whose counter held counter0"""
    return (counter0 + 1, counter0 + 2)


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def noisy_cases():
    """every (net, seed, call) the floors and caps run over"""
    for net in NETS:
        for seed, c0 in SEED_CASES:
            for call in calls(c0):
                yield net, seed, call


@functools.lru_cache(maxsize=None)
def reference(net, sd, action_sd, seed, call, squares, dtype="float64"):
    """the restated actions of all ROWS rows (read-only, computed once)"""
    out = noise_ref.actor_forward_noisy(params(net), inputs(), sd, action_sd, seed, call, 0, squares,
                                        getattr(np, dtype))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def floors():
    f = {}
    for sd in SDS:
        for sq in ("exact", "bf16"):
            f[sq, sd] = max(_maxdiff(reference(net, sd, asd, seed, call, sq, "float32"),
                                     reference(net, sd, asd, seed, call, sq))
                            for net, seed, call in noisy_cases() for asd in (0.0, ACTION_SD))
    rows = np.arange(ROWS)
    f["z"] = max(_maxdiff(noise_ref.action_normals(seed, call, rows, np.float32),
                          noise_ref.action_normals(seed, call, rows))
                 for _, seed, call in noisy_cases())
    f["clean"] = max(_maxdiff(reference(net, 0.0, 0.0, 0, 0, "exact", "float32"),
                              reference(net, 0.0, 0.0, 0, 0, "exact")) for net in NETS)
    return f


@functools.lru_cache(maxsize=None)
def caps():
    """1/4 of the least max-deviation of the 1 %-sd mutant: per sd over nets,
    seeds, calls and both squares; 'z': action_sd x 1.01 on the normals"""
    c = {}
    for sd in SDS:
        c[sd] = 0.25 * min(_maxdiff(noise_ref.actor_forward_noisy(params(net), inputs(), sd * 1.01, 0.0, seed, call,
                                                                  0, sq),
                                    reference(net, sd, 0.0, seed, call, sq))
                           for net, seed, call in noisy_cases() for sq in ("exact", "bf16"))
    rows = np.arange(ROWS)
    c["z"] = 0.25 * min(0.01 * float(np.abs(noise_ref.action_normals(seed, call, rows)).max())
                        for _, seed, call in noisy_cases())
    return c


def bars():
    """{('exact' | 'bf16', sd): bar, 'z': bar on the normals, 'clean': noise-free bar}"""
    f = floors()
    b = {k: FACTOR * v for k, v in f.items() if k != "clean"}
    b["clean"] = CLEAN_FACTOR * f["clean"]
    return b


@functools.lru_cache(maxsize=None)
def clean_reference(net):
    out, _ = keras_ref.actor_forward(params(net), inputs().astype(np.float64))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dropped_deviations():
    """max |split forward without one class of piece products - fp64 forward|,
    the least over both nets, per class; 'full': the six-product model's own
    (the largest over both nets)"""
    d = {}
    for name, pr in DROPPED.items():
        keep = tuple(p for p in noise_ref.SPLIT_PRODUCTS if p != pr)
        d[name] = min(_maxdiff(noise_ref.split_forward(params(net), inputs(), keep), clean_reference(net))
                      for net in NETS)
    d["full"] = max(_maxdiff(noise_ref.split_forward(params(net), inputs()), clean_reference(net)) for net in NETS)
    return d
