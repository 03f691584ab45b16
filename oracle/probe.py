"""ctypes binding of the numeric probes (oracle/sk_probe.hip).

TEST INFRASTRUCTURE ONLY.  Two libraries built from the one source by
oracle/Makefile: `libsk_probe.so` (hipcc with the product's flag list; kernels
over device pointers) and `libsk_probe_host.so` (g++ like the host checks; the
same wrappers of the host-compilable headers over host pointers).  Both wrap
the product's own functions element by element and add no arithmetic.

    run_host("trig", x=angles, d=steps)      -> dict of numpy arrays
    run_device("trig", x=angles, d=steps)    -> the same from the GPU

Inputs not given are zeros; an array of k-tuples is given as [k, n].
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "_build")
# SK_PROBE_LIB: a differently built device library (the headers at another revision)
DEVICE_LIB = os.environ.get("SK_PROBE_LIB") or os.path.join(_BUILD, "libsk_probe.so")
HOST_LIB = os.path.join(_BUILD, "libsk_probe_host.so")
MAX_ELEMENTS = 1 << 20  # per launch

RANGE_PREDICATES = ("cfg_ok", "fits_axis", "fits_board", "box_hit", "pair_h1", "pair_h2", "pack_fits_player",
                    "pack_fits_game", "admit_cfg", "admit_player", "admit_game")

# group -> (inputs, outputs, the outputs the host twin fills or None for a device-only group): (name, dtype,
# planes) in the order of sk_probe.hip's skp_<group>_args
GROUPS = {
    "trig": ((("x", "f8", 1), ("d", "f4", 1), ("speed", "f4", 1), ("act", "f4", 1), ("rs_d", "f4", 1),
              ("rs_eps", "f4", 1), ("look", "f8", 1)),
             (("bf_s", "f8", 1), ("bf_c", "f8", 1), ("fast_s", "f4", 1), ("fast_c", "f4", 1), ("add_s", "f4", 1),
              ("add_c", "f4", 1), ("move_x", "f4", 1), ("move_y", "f4", 1), ("step_x", "f4", 1), ("step_y", "f4", 1),
              ("bf_ok", "u1", 1), ("fast_ok", "u1", 1), ("rs", "u1", 1), ("move_safe", "u1", 1),
              ("step_safe", "u1", 1), ("look_fits", "u1", 1)),
             "all"),
    "tan": ((("x", "f8", 1),),
            (("tan_cr", "f8", 1), ("grad_cr", "f8", 1), ("grad_fast", "f8", 1), ("tan_lib", "f8", 1)),
            ("tan_cr",)),
    "lib": ((("x", "f8", 1),), (("s", "f8", 1), ("c", "f8", 1)), None),
    "range": ((("v", "i4", 8),), (("out", "u1", len(RANGE_PREDICATES)),), "all"),
    "feat": ((("r", "f8", 1), ("p", "i4", 4), ("g", "f8", 1), ("a", "f8", 1), ("af", "f4", 1)),
             (("mod2", "f8", 1), ("mod2_fast", "f8", 1), ("dpp", "f8", 1), ("dlp", "f8", 1), ("clamp", "f8", 1),
              ("clamp_f", "f4", 1)),
             None),
    "rng": ((("ctr", "u4", 4), ("key", "u4", 2), ("u", "u4", 1), ("lo", "i4", 1), ("hi", "i4", 1)),
            (("out", "u4", 4), ("action", "f4", 1), ("pos", "i4", 1)),
            None),
}

_libs = {}


def _make(target):
    subprocess.run(["make", "-s", "-C", _HERE, os.path.join("_build", os.path.basename(target))], check=True)


def _load(path):
    if path not in _libs:
        src = os.path.join(_HERE, "sk_probe.hip")
        if os.path.dirname(path) == _BUILD and (not os.path.exists(path) or
                                                os.path.getmtime(path) < os.path.getmtime(src)):
            _make(path)
        L = ctypes.CDLL(path)
        for group, (_, _, host) in GROUPS.items():
            if path == HOST_LIB:
                if host is not None:
                    fn = getattr(L, f"skp_{group}_host")
                    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int64], ctypes.c_int
            else:
                fn = getattr(L, f"skp_{group}")
                fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p], ctypes.c_int
        _libs[path] = L
    return _libs[path]


def _inputs(group, given):
    """-> (n, [contiguous numpy array per input]) with missing inputs zero"""
    ins = GROUPS[group][0]
    unknown = set(given) - {name for name, _, _ in ins}
    if unknown:
        raise TypeError(f"{group}: no input {sorted(unknown)}")
    if not given:
        raise TypeError(f"{group}: no input given")
    n = None
    for name, _, planes in ins:
        if name in given:
            a = np.asarray(given[name])
            m = a.shape[-1] if planes > 1 else a.size
            if n is not None and m != n:
                raise ValueError(f"{group}: {name} has {m} elements, others {n}")
            n = m
    if n > MAX_ELEMENTS:
        raise ValueError(f"{group}: {n} elements, at most {MAX_ELEMENTS} per launch")
    arrays = []
    for name, dt, planes in ins:
        shape = (planes, n) if planes > 1 else (n,)
        if name in given:
            a = np.asarray(given[name])
            if a.dtype != np.dtype(dt):
                raise TypeError(f"{group}: {name} must be {np.dtype(dt)}, got {a.dtype}")
            a = np.ascontiguousarray(a).reshape(shape)
        else:
            a = np.zeros(shape, dt)
        arrays.append(a)
    return n, arrays


def _struct(pointers):
    return (ctypes.c_void_p * len(pointers))(*pointers)  # a struct of pointers, in field order


def run_host(group, **given):
    ins, outs, host = GROUPS[group]
    if host is None:
        raise ValueError(f"{group}: device-only group")
    n, arrays = _inputs(group, given)
    res = [np.zeros((planes, n) if planes > 1 else (n,), dt) for _, dt, planes in outs]
    args = _struct([a.ctypes.data for a in arrays + res])
    status = getattr(_load(HOST_LIB), f"skp_{group}_host")(ctypes.addressof(args), n)
    assert status == 0, status
    return {name: r for (name, _, _), r in zip(outs, res) if host == "all" or name in host}


def run_device(group, **given):
    import torch  # before the library: one HIP runtime per process (skillshot_learning_amd/_capi.py)
    L = _load(DEVICE_LIB)
    ins, outs, _ = GROUPS[group]
    n, arrays = _inputs(group, given)
    dev = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in arrays]
    res = [torch.zeros(max(1, planes * n * np.dtype(dt).itemsize), dtype=torch.uint8, device="cuda")
           for _, dt, planes in outs]
    dev = [t if t.numel() else torch.zeros(1, dtype=torch.uint8, device="cuda") for t in dev]
    args = _struct([t.data_ptr() for t in dev + res])
    stream = torch.cuda.current_stream().cuda_stream
    status = getattr(L, f"skp_{group}")(ctypes.addressof(args), n, stream)
    torch.cuda.synchronize()
    if status != 0:
        raise RuntimeError(f"skp_{group}: HIP status {status}")
    out = {}
    for (name, dt, planes), t in zip(outs, res):
        a = t.cpu().numpy()[:planes * n * np.dtype(dt).itemsize].view(dt)
        out[name] = a.reshape((planes, n) if planes > 1 else (n,)).copy()
    return out
