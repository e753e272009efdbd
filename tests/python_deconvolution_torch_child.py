"""The AlgorithmType.python cases that hand device memory to torch, run in a
process of their own by tests/test_python_deconvolution_gpu.py:

    python tests/python_deconvolution_torch_child.py RESULTS.json [case ...]

Why a process of their own: a DLPack tensor is a bare device pointer, so its
producer (librdl_hip) and its consumer (torch) must share one HIP runtime.
PyTorch wheels for ROCm bundle a HIP runtime of their own, with the system
runtime's soname but another file name. Imported after radler, torch loads
that second runtime, which finds no device in a process whose first runtime
holds it. Imported first, its runtime is the one librdl_hip's dependency
resolves to, and the process has one. The pytest process has imported radler
long before this module's tests run; this process imports torch first.

Every case is a function that asserts; RESULTS.json maps each case's name to
null (passed) or its traceback.
"""
import torch  # first: see above

import gc
import json
import pathlib
import sys
import tempfile
import traceback

import numpy as np

from python_deconvolution_lib import (GRID_DEVICE, HEIGHT, N_FREQ, N_POL, TORCH_CASES, WIDTH,
                                      Joined, check_grid, expect_bad_return, make_inputs,
                                      probe_module, write)

DEVICE_PRELUDE = "    import torch\n    r = torch.from_dlpack(residual)\n"
BAD_RETURNS = {
    "wrong_shape": (DEVICE_PRELUDE + '    return {"level": 0.0, "continue": False, '
                    '"model": r[:, :, :-1, :].contiguous()}',
                    r"'model'.*shape \(1, 1, 23, 40\).*\(1, 1, 24, 40\)"),
    "float64": (DEVICE_PRELUDE + '    return {"level": 0.0, "continue": False, '
                '"residual": r.double()}', "'residual'.*float32"),
    "non_contiguous": (DEVICE_PRELUDE + "    wide = torch.zeros(1, 1, 24, 80, device=r.device)\n"
                       '    return {"level": 0.0, "continue": False, "residual": wide[..., ::2]}',
                       "'residual'.*not C-contiguous"),
    "cpu": (DEVICE_PRELUDE + '    return {"level": 0.0, "continue": False, "residual": r.cpu()}',
            "'residual'.*device"),
}

DEVICE_FILE = """
import torch
import radler_python_probe as probe


def deconvolve_device(residual, model, psf, meta):
    arrays = dict(residual=residual, model=model, psf=psf)
    tensors = {k: torch.from_dlpack(a) for k, a in arrays.items()}
    probe.calls.append(dict(
        array_types={k: type(a).__name__ for k, a in arrays.items()},
        array_shapes={k: a.shape for k, a in arrays.items()},
        array_dtypes={k: a.dtype for k, a in arrays.items()},
        dlpack_devices={k: a.__dlpack_device__() for k, a in arrays.items()},
        devices={k: (t.device.type, t.device.index) for k, t in tensors.items()},
        dtypes={k: t.dtype for k, t in tensors.items()},
        shapes={k: tuple(t.shape) for k, t in tensors.items()},
        strides={k: t.stride() for k, t in tensors.items()},
        pointers={k: t.data_ptr() for k, t in tensors.items()},
        copies={k: t.cpu().numpy().copy() for k, t in tensors.items()},
        max_iterations=meta.max_iterations,
    ))
    r, m = tensors["residual"], tensors["model"]
BODY
"""
IN_PLACE = """
    m.add_(r, alpha=0.5)
    r.mul_(0.25)
    return RETURN
"""
IN_PLACE_RETURNS = {
    "level_and_continue": '{"level": 0.25, "continue": False}',
    "none": '{"level": 0.25, "continue": False, "residual": None, "model": None}',
    "the_views": '{"level": 0.25, "continue": False, "residual": residual, "model": model}',
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_device_call(call, inputs):
    residual, model, psf = inputs
    image_shape = (N_FREQ, N_POL, HEIGHT, WIDTH)
    shapes = dict(residual=image_shape, model=image_shape, psf=(N_FREQ, HEIGHT, WIDTH))
    assert set(call["array_types"].values()) == {"DeviceArray"}
    assert call["array_shapes"] == shapes and call["shapes"] == shapes
    assert set(call["array_dtypes"].values()) == {"float32"}
    device = torch.cuda.current_device()
    assert set(call["dlpack_devices"].values()) == {(10, device)}  # kDLROCM
    assert set(call["devices"].values()) == {("cuda", device)}
    assert set(call["dtypes"].values()) == {torch.float32}
    plane = HEIGHT * WIDTH
    assert call["strides"]["residual"] == call["strides"]["model"] == \
        (N_POL * plane, plane, WIDTH, 1)
    assert call["strides"]["psf"] == (plane, WIDTH, 1)
    assert len(set(call["pointers"].values())) == 3
    for name, expect in (("residual", residual), ("model", model), ("psf", psf)):
        assert np.array_equal(call["copies"][name], expect), name


def in_place(returns):
    def case(directory, probe, inputs):
        body = IN_PLACE.replace("RETURN", IN_PLACE_RETURNS[returns])
        run = Joined(inputs, write(directory, DEVICE_FILE.replace("BODY", body)))
        assert run.radler.perform(1) is False
        assert len(probe.calls) == 1
        check_device_call(probe.calls[0], inputs)
        assert probe.calls[0]["max_iterations"] == run.settings.minor_iteration_count
        residual, model, psf = inputs
        # both exact in float32, fused or not: 0.5 * r and 0.25 * r are exact,
        # and m + 0.5 * r rounds once either way
        assert np.array_equal(bits(run.residual), bits(np.float32(0.25) * residual))
        assert np.array_equal(bits(run.model), bits(model + np.float32(0.5) * residual))
        assert np.array_equal(run.psf, psf)
    return case


def returned_copy(directory, probe, inputs):
    """A fresh tensor under 'residual' is copied device to device; the model
    view, edited in place, is kept."""
    body = """
    m.add_(r, alpha=0.5)
    return {"level": 0.25, "continue": True, "residual": r.clone().mul_(0.5)}
"""
    run = Joined(inputs, write(directory, DEVICE_FILE.replace("BODY", body)))
    assert run.radler.perform(1) is True
    check_device_call(probe.calls[0], inputs)
    residual, model, psf = inputs
    assert np.array_equal(bits(run.residual), bits(np.float32(0.5) * residual))
    assert np.array_equal(bits(run.model), bits(model + np.float32(0.5) * residual))


def tensors_outlive_the_call(directory, probe, inputs):
    """Tensors the user keeps hold the image sets' allocation through their
    DLPack capsules: after perform(), and after the Radler object is gone, one
    read of them succeeds. Their contents are stale, not freed."""
    path = write(directory, """
import torch
import radler_python_probe as probe


def deconvolve_device(residual, model, psf, meta):
    probe.kept.extend(torch.from_dlpack(a) for a in (residual, model, psf))
    probe.kept.append(residual)
    return {"level": 0.0, "continue": False}
""")
    run = Joined(inputs, path)
    assert run.radler.perform(1) is False
    del run
    gc.collect()
    assert len(probe.kept) == 4
    for tensor in probe.kept[:3]:
        assert bool(torch.isfinite(tensor.cpu()).all())
    # the view itself still exports
    assert bool(torch.isfinite(torch.from_dlpack(probe.kept[3]).cpu()).all())
    probe.kept.clear()
    gc.collect()


def bad_return(name):
    def case(directory, probe, inputs):
        expect_bad_return(directory, "deconvolve_device", *BAD_RETURNS[name])
    return case


def grid(max_threads):
    def case(directory, probe, inputs):
        check_grid(directory, probe, max_threads, GRID_DEVICE)
    return case


CASES = {
    **{f"bad_return_{name}": bad_return(name) for name in BAD_RETURNS},
    **{f"in_place_{name}": in_place(name) for name in IN_PLACE_RETURNS},
    "returned_copy": returned_copy,
    "tensors_outlive_the_call": tensors_outlive_the_call,
    "grid_in_turn": grid(1),
    "grid_pooled": grid(2),
}
assert set(CASES) == set(TORCH_CASES)


def main(results_path, names):
    results = {}
    try:
        assert torch.cuda.is_available(), "torch sees no GPU"
        inputs = make_inputs()
        for name in names or TORCH_CASES:
            with tempfile.TemporaryDirectory() as directory, probe_module() as probe:
                try:
                    CASES[name](pathlib.Path(directory), probe, inputs)
                    results[name] = None
                except Exception:  # noqa: BLE001
                    results[name] = traceback.format_exc()
            print(name, "ok" if results[name] is None else "FAILED", flush=True)
    except Exception:  # noqa: BLE001
        results["child"] = traceback.format_exc()
    with open(results_path, "w") as f:
        json.dump(results, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
