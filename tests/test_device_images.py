"""What device images promise without a device: DeviceImageAccessor's
properties, its read-only check, its keep-alive, and the checks a Radler makes
when it is constructed over device accessors (tests/device_accessor_cxx_host.cc,
mode `cpu`); and the Python side's refusal of what is no image at all."""
import os
import subprocess

import numpy as np
import pytest

from radler_fixtures import BEAM_SIZE, get_psf, get_residual, make_settings
from radler_import import radler as rd
from test_subminor_plan import _host_build

HERE = os.path.dirname(os.path.abspath(__file__))


def build_cxx_host(directory):
    b = _host_build()
    exe = str(directory / "device_accessor_cxx_host")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "device_accessor_cxx_host.cc"),
                    "-o", exe, f"-L{b.LIB}", "-lradler_amd", "-lrdl_hip",
                    f"-Wl,-rpath,{b.LIB}"], check=True)
    return exe


def test_accessor_properties_and_construction_checks(tmp_path):
    host = subprocess.run([build_cxx_host(tmp_path), "cpu"], capture_output=True, text=True)
    assert host.returncode == 0 and host.stdout.strip() == "OK", host.stdout + host.stderr


def test_device_array_api_is_there():
    assert callable(rd.gpu.to_device)
    for name in ("numpy", "view", "data_ptr", "shape", "__dlpack__", "__dlpack_device__"):
        assert hasattr(rd.gpu.DeviceArray, name), name
    assert "__dlpack__" in rd.Radler.__doc__ and "torch" in rd.Radler.__doc__
    assert "device arrays" in rd.Settings.Python.__doc__


class HostTensor:
    """A DLPack producer on the CPU: refused by its __dlpack_device__ alone."""

    def __init__(self):
        self.exported = 0

    def __dlpack_device__(self):
        return (1, 0)

    def __dlpack__(self, stream=None):
        self.exported += 1
        raise AssertionError("a host tensor must not be exported")


def test_objects_that_are_no_images_are_type_errors():
    settings = make_settings()
    psf, residual = get_psf(), get_residual(1.0, 0, 0)
    model = np.zeros_like(residual)
    with pytest.raises(TypeError, match="'residual' is a list"):
        rd.Radler(settings, psf, [[0.0]], model, BEAM_SIZE)
    with pytest.raises(TypeError, match="'psf' is a numpy.ndarray that is no float32"):
        rd.Radler(settings, psf.astype(np.float64), residual, model, BEAM_SIZE)
    with pytest.raises(TypeError, match="'model' is a numpy.ndarray that is no float32"):
        rd.Radler(settings, psf, residual, model.T, BEAM_SIZE)
    tensor = HostTensor()
    with pytest.raises(TypeError, match=r"'model' is on DLPack device \(1, 0\), not on a ROCm"):
        rd.Radler(settings, psf, residual, tensor, BEAM_SIZE)
    assert tensor.exported == 0
    entry = rd.WorkTableEntry()
    with pytest.raises(TypeError, match=r"'residual' is on DLPack device \(1, 0\)"):
        entry.residual = tensor
    with pytest.raises(TypeError, match="'psf'"):
        entry.psfs.append(tensor)
    with pytest.raises(TypeError, match="'model' is a str"):
        entry.model = "model.fits"
    rd.Radler(settings, psf, residual, model, BEAM_SIZE)
