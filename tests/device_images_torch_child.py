"""The device-image cases on torch tensors, run in a process of their own by
tests/test_device_images_gpu.py:

    python tests/device_images_torch_child.py RESULTS.json [case ...]

Why a process of their own: as python_deconvolution_torch_child.py explains, a
DLPack tensor is a bare device pointer, so torch and librdl_hip must share one
HIP runtime, which they do only when torch is imported first. The pytest
process imported radler long ago; this one imports torch first.

Every case is a function that asserts; RESULTS.json maps each case's name to
null (passed) or its traceback.
"""
import torch  # first: see above

import json
import re
import sys
import traceback

import numpy as np

import device_images_lib as L
from radler_import import radler as rd


class TorchBackend:
    @staticmethod
    def to_device(array):
        return torch.from_numpy(np.ascontiguousarray(array, np.float32)).to("cuda")

    @staticmethod
    def to_host(tensor):
        torch.cuda.synchronize()
        return tensor.cpu().numpy()

    @staticmethod
    def pointer(tensor):
        return tensor.data_ptr()

    @staticmethod
    def plane(tensor, index):
        return tensor[index]


def all_three_tensors():
    psf, residual, model = L.inputs(1)
    L.compare(L.simple(L.settings()), psf[0], residual[0], model[0], backend=TorchBackend)


def produced_on_another_stream():
    """The residual is the last operation of a long queue on a stream of
    torch's that nobody waits for: perform() itself must (rdl_device_sync
    before its first read), whatever stream the tensor came from."""
    psf, residual, model = L.inputs(1)
    stream = torch.cuda.Stream()

    def make_device(name, array):
        tensor = TorchBackend.to_device(array)
        if name != "residual":
            return tensor
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            busy = torch.zeros(4096, 4096, device="cuda")
            for _ in range(30):
                busy = busy @ busy
            produced = torch.full_like(tensor, float("nan"))
            produced.copy_(tensor + busy[0, 0])          # + 0.0, after the queue
        return produced

    L.compare(L.simple(L.settings()), psf[0], residual[0], model[0], backend=TorchBackend,
              make_device=make_device)


def channels_polynomial():
    build, psf, residual, model = L.channels_case(rd.SpectralFittingMode.polynomial)
    L.compare(build, psf, residual, model, backend=TorchBackend)


def work_table_of_tensor_slices():
    """tensor[index]: views with a storage offset, through the entry setters."""
    build, psf, residual, model = L.polarizations_case(TorchBackend)
    L.compare(build, psf, residual, model, backend=TorchBackend)


def expect(error, message, make):
    try:
        make()
    except error as e:
        assert re.search(message, str(e)), str(e)
    else:
        raise AssertionError("accepted")


def error_case(which):
    def case():
        psf, residual, model = (TorchBackend.to_device(a[0]) for a in L.inputs(1))
        s = L.settings()
        if which == "float64":
            expect(TypeError, r"'residual' has dtype \(code 2, 64 bits\), float32 is required",
                   lambda: rd.Radler(s, psf, residual.double(), model, L.BEAM))
        elif which == "non_contiguous":
            wide = torch.zeros(L.HEIGHT, 2 * L.WIDTH, device="cuda")
            expect(TypeError, r"'psf' is not C-contiguous \(shape \(48, 64\), strides \(128, 2\)",
                   lambda: rd.Radler(s, wide[:, ::2], residual, model, L.BEAM))
        elif which == "cpu_tensor":
            expect(TypeError, r"'model' is on DLPack device .*not on a ROCm device",
                   lambda: rd.Radler(s, psf, residual, model.cpu(), L.BEAM))
        elif which == "other_device" and torch.cuda.device_count() > 1:
            expect(RuntimeError, r"residual image of entry 0 is on HIP device 1, the "
                                 r"deconvolution runs on device 0",
                   lambda: rd.Radler(s, psf, residual.to("cuda:1"), model, L.BEAM))
        # the refused arguments are untouched and still usable
        rd.Radler(s, psf, residual, model, L.BEAM).perform(1)
    return case


CASES = {
    "all_three_tensors": all_three_tensors,
    "produced_on_another_stream": produced_on_another_stream,
    "channels_polynomial": channels_polynomial,
    "work_table_of_tensor_slices": work_table_of_tensor_slices,
    **{f"error_{name}": error_case(name)
       for name in ("float64", "non_contiguous", "cpu_tensor", "other_device")},
}


def main(results_path, names):
    results = {}
    try:
        assert torch.cuda.is_available(), "torch sees no GPU"
        for name in names or CASES:
            try:
                CASES[name]()
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
