"""AlgorithmType.python (csrc/python/python_deconvolution.cc; reference:
cpp/algorithms/python_deconvolution.cc, cpp/test/test_python_deconvolution.cc):
what is decided when the Radler object is made, which needs no device. The
user's file is evaluated then, and every way it can fail becomes a RuntimeError
carrying Python's message. The host libraries stay free of libpython: the
algorithm lives in the Python module and reaches libradler_amd through a
factory hook.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from radler_import import radler as rd
from rdl_lib import HIP_SO, PKG

WIDTH, HEIGHT = 40, 24


def make_radler(filename):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.python
    s.python.filename = str(filename)
    s.trimmed_image_width, s.trimmed_image_height = WIDTH, HEIGHT
    s.pixel_scale.x = s.pixel_scale.y = 1.0 / 60.0 * np.pi / 180.0
    s.minor_iteration_count = 1000
    s.absolute_threshold = 1.0e-8
    psf = np.zeros((HEIGHT, WIDTH), np.float32)
    return rd.Radler(s, psf, psf.copy(), psf.copy(), 0.0)


def write(tmp_path, text, name="deconvolve_file.py"):
    path = tmp_path / name
    path.write_text(text)
    return path


def test_missing_file(tmp_path):
    with pytest.raises(RuntimeError, match="no_such_file.py"):
        make_radler(tmp_path / "no_such_file.py")


def test_file_that_raises(tmp_path):
    path = write(tmp_path, '#! /usr/bin/python\n\n'
                           'raise RuntimeError("This should give an error during construction")\n')
    with pytest.raises(RuntimeError, match="This should give an error during construction"):
        make_radler(path)


def test_syntax_error(tmp_path):
    path = write(tmp_path, "def deconvolve(residual, model, psf, meta)\n    return {}\n")
    with pytest.raises(RuntimeError, match="SyntaxError") as e:
        make_radler(path)
    assert "deconvolve_file.py" in str(e.value)


def test_file_without_a_function(tmp_path):
    path = write(tmp_path, "import numpy\n\ndef clean(residual, model, psf, meta):\n    pass\n")
    with pytest.raises(RuntimeError) as e:
        make_radler(path)
    message = str(e.value)
    assert "deconvolve(" in message and "deconvolve_device(" in message
    assert "not available" not in message


def test_file_is_evaluated_once_in_its_own_namespace(tmp_path):
    import sys
    import types
    probe = types.ModuleType("radler_python_probe")
    probe.seen = []
    sys.modules["radler_python_probe"] = probe
    try:
        path = write(tmp_path, "import radler_python_probe\n"
                               "radler_python_probe.seen.append((__name__, __file__))\n"
                               "marker_of_the_user_file = 1\n"
                               "def deconvolve(residual, model, psf, meta):\n    pass\n")
        radler = make_radler(path)
        assert len(probe.seen) == 1
        name, file = probe.seen[0]
        assert name != "__main__" and file == str(path)
        assert not hasattr(sys.modules["__main__"], "marker_of_the_user_file")
        del radler
    finally:
        del sys.modules["radler_python_probe"]


def test_helper_classes_are_registered_once():
    assert {"Channel", "MetaData", "SpectralFitter"} <= set(dir(rd.python_deconvolution))
    assert hasattr(rd.gpu, "DeviceArray")
    assert "deconvolve_device" in rd.Settings.Python.__doc__


def test_cxx_host_without_the_module_is_told_what_is_missing(tmp_path):
    """tests/python_deconvolution_cxx_host.cc: libradler_amd.so alone has no
    factory for the algorithm and says that the Python module is needed."""
    from test_subminor_plan import _host_build
    b = _host_build()
    exe = str(tmp_path / "cxx_host")
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(here, "python_deconvolution_cxx_host.cc"),
                    "-o", exe, f"-L{b.LIB}", "-lradler_amd", "-lrdl_hip",
                    f"-Wl,-rpath,{b.LIB}"], check=True)
    host = subprocess.run([exe], capture_output=True, text=True)
    assert host.returncode == 0, host.stdout + host.stderr
    assert "radler Python module" in host.stdout and "loaded in the process" in host.stdout


def needed_libraries(path):
    """DT_NEEDED entries of an ELF64 little-endian shared object."""
    readelf = shutil.which("readelf")
    if readelf:
        out = subprocess.run([readelf, "-d", path], capture_output=True, text=True, check=True)
        return [line.split("[")[1].split("]")[0] for line in out.stdout.splitlines()
                if "(NEEDED)" in line]
    raw = open(path, "rb").read()
    assert raw[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", raw, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", raw, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", raw, shoff + i * shentsize)
                for i in range(shnum)]
    needed = []
    for section in sections:
        if section[1] != 6:  # SHT_DYNAMIC
            continue
        strtab = sections[section[6]]  # sh_link
        for at in range(section[4], section[4] + section[5], 16):
            tag, value = struct.unpack_from("<qQ", raw, at)
            if tag == 0:
                break
            if tag == 1:  # DT_NEEDED
                start = strtab[4] + value
                needed.append(raw[start:raw.index(b"\0", start)].decode())
    return needed


@pytest.mark.parametrize("library", [os.path.join(PKG, "lib", "libradler_amd.so"), HIP_SO])
def test_host_libraries_do_not_need_libpython(library):
    needed = needed_libraries(library)
    assert needed, "no DT_NEEDED entries read"
    assert not [n for n in needed if "python" in n.lower()], needed
