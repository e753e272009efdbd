"""radler.Radler over images that already live in device memory.

Every case builds two Radlers from the same data, one over numpy arrays and
one over radler.gpu.to_device arrays, runs perform(1) and perform(2) on both
and requires the same flags, iteration numbers, residual and model bits and
component lists, an untouched PSF and device arrays that stayed where they
were (device_images_lib.compare). The host run is the parent behaviour: that
path is unchanged.

The cases on torch tensors run in one child process that imports torch first
(device_images_torch_child.py, for the reason given there); the C++ host of
tests/device_accessor_cxx_host.cc is built and run here.
"""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import device_images_lib as L
from device_images_lib import RadlerBackend, compare
from radler_import import radler as rd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_CASES = ["all_three_tensors", "produced_on_another_stream", "channels_polynomial",
               "work_table_of_tensor_slices", "error_float64", "error_non_contiguous",
               "error_cpu_tensor", "error_other_device"]


def test_hogbom_one_image():
    psf, residual, model = L.inputs(1)
    compare(L.simple(L.settings()), psf[0], residual[0], model[0])


@pytest.mark.parametrize("fitting", [None, "polynomial", "log_polynomial"])
def test_four_channels_in_two_groups(fitting):
    """Unequal weights, one 0 on a residual of NaNs. No fitting stores each
    group's model into its channels as it is; the fitted modes interpolate
    (rdl_spectral_interpolate / rdl_logpoly_interpolate) and store from the
    interpolation's output planes."""
    mode = getattr(rd.SpectralFittingMode, fitting) if fitting else None
    build, psf, residual, model = L.channels_case(mode)
    of_host, of_device, mixed = compare(build, psf, residual, model)
    # the NaN plane was never read, and was overwritten with its group's residual
    assert np.isfinite(mixed["residual"].numpy()).all()


def test_two_linked_polarizations_through_entry_setters():
    build, psf, residual, model = L.polarizations_case()
    compare(build, psf, residual, model)


def test_multiscale_on_a_grid_with_two_threads():
    build, psf, residual, model = L.multiscale_grid_case()
    compare(build, psf, residual, model)


@pytest.mark.parametrize("device", [("residual", "model"), ("psf",), ("psf", "model")])
def test_host_and_device_images_mixed(device):
    """A host PSF with device images (the likely case), the reverse, and a
    model alone: per plane, whichever kind it is."""
    build, psf, residual, model = L.channels_case(rd.SpectralFittingMode.polynomial)
    compare(build, psf, residual, model, device=device)


def test_mixed_kinds_inside_one_deconvolution_group():
    """Channels 0 and 1 share a group: a host accessor next to a device one
    sends that plane through the chain, with the device plane fed to rdl_axpy
    where it is; group 1 (all device) takes the fused kernel."""
    psf, residual, model = L.inputs(4)
    s = L.settings()
    on_host = {("residual", 0), ("psf", 1), ("model", 1)}

    def plane(name, stack, index):
        if isinstance(stack, np.ndarray) or (name, index) in on_host:
            host = stack[index] if isinstance(stack, np.ndarray) else kept[name][index]
            return host
        return RadlerBackend.plane(stack, index)

    kept = {}

    def build(psf, residual, model):
        stacks = dict(psf=psf, residual=residual, model=model)
        if not isinstance(psf, np.ndarray):
            # host copies for the planes that stay on the host in the mixed table
            kept.update({k: v.numpy() for k, v in stacks.items()})
        table = rd.WorkTable([], 4, 2)
        for c in range(4):
            e = rd.WorkTableEntry()
            e.original_channel_index = c
            e.band_start_frequency, e.band_end_frequency = L.BANDS[c]
            e.image_weight = [1.0, 2.0, 0.5, 1.5][c]
            e.psfs.append(plane("psf", psf, c))
            e.residual = plane("residual", residual, c)
            e.model = plane("model", model, c)
            table.add_entry(e)
        return rd.Radler(s, table, L.BEAM)

    host = {k: v.copy() for k, v in dict(psf=psf, residual=residual, model=model).items()}
    device = {k: RadlerBackend.to_device(v) for k, v in host.items()}
    of_host, of_device = build(**host), build(**device)
    for major in (1, 2):
        assert of_host.perform(major) == of_device.perform(major)
        assert of_host.iteration_number == of_device.iteration_number
        for name in ("residual", "model"):
            got = device[name].numpy()
            for c in range(4):
                if (name, c) in on_host:
                    got[c] = kept[name][c]
            assert np.array_equal(L.bits(got), L.bits(host[name])), (name, major)
    assert of_host.iteration_number > 0
    assert L.components(of_host) == L.components(of_device)


def test_residual_as_a_view_four_bytes_into_a_larger_array():
    psf, residual, model = L.inputs(1)
    views = {}

    def make_device(name, array):
        if name != "residual":
            return RadlerBackend.to_device(array)
        big = rd.gpu.to_device(np.concatenate([[np.float32(7.0)], array.ravel(),
                                               [np.float32(9.0)]]).astype(np.float32))
        views["big"] = big
        view = big.view(1, array.shape)
        assert view.data_ptr == big.data_ptr + 4 and view.data_ptr % 16 == 4
        return view

    compare(L.simple(L.settings()), psf[0], residual[0], model[0], make_device=make_device)
    ends = views["big"].numpy()
    assert ends[0] == 7.0 and ends[-1] == 9.0


def test_byte_offset_of_a_producer_is_honoured():
    psf, residual, model = L.inputs(1)
    height, width = residual[0].shape
    producers = {}

    class Backend(RadlerBackend):
        @staticmethod
        def to_host(producer):
            return producer.array.numpy().ravel()[1:1 + height * width].reshape(height, width)

        @staticmethod
        def pointer(producer):
            return producer.array.data_ptr

    def make_device(name, array):
        big = rd.gpu.to_device(np.concatenate([[np.float32(0.0)], array.ravel()])
                               .astype(np.float32))
        producers[name] = L.CountingProducer(big, shape=array.shape, byte_offset=4)
        return producers[name]

    compare(L.simple(L.settings()), psf[0], residual[0], model[0], backend=Backend,
            make_device=make_device)


def test_the_radler_keeps_the_device_memory_alive():
    """The caller drops every reference after construction: perform() still
    works on live memory, and the three tensors are given back (their deleters
    run) when the Radler is destroyed, not before."""
    psf, residual, model = L.inputs(1)
    expected = compare(L.simple(L.settings()), psf[0], residual[0], model[0])[2]
    want_residual = expected["residual"].numpy()
    del expected
    gc.collect()
    live_before = len(L.CountingProducer.live)
    counts = dict(exported=0, deleted=0)
    arrays = [rd.gpu.to_device(a[0]) for a in (psf, residual, model)]
    producers = [L.CountingProducer(a, counts=counts) for a in arrays]
    watch = arrays[1].view(0, arrays[1].shape)   # a second view, to read the result through
    radler = rd.Radler(L.settings(), *producers, L.BEAM)
    assert counts == dict(exported=3, deleted=0)
    del arrays, producers
    gc.collect()
    assert len(L.CountingProducer.live) == live_before + 3
    # other allocations may now land where freed memory would be
    churn = [rd.gpu.to_device(np.full((L.HEIGHT, L.WIDTH), np.nan, np.float32))
             for _ in range(4)]
    radler.perform(1)
    radler.perform(2)
    assert counts["deleted"] == 0
    assert np.array_equal(L.bits(watch.numpy()), L.bits(want_residual))
    del radler, churn
    gc.collect()
    assert counts == dict(exported=3, deleted=3)
    assert len(L.CountingProducer.live) == live_before


def test_errors_name_the_argument_and_the_requirement():
    psf, residual, model = (RadlerBackend.to_device(a[0]) for a in L.inputs(1))
    s = L.settings()
    small = rd.gpu.to_device(np.zeros((L.HEIGHT - 1, L.WIDTH), np.float32))
    with pytest.raises(RuntimeError, match=r"equal shape: psf \(48, 64\), residual \(47, 64\)"):
        rd.Radler(s, psf, small, model, L.BEAM)
    with pytest.raises(RuntimeError, match="residual image of entry 0 .* overlaps the model "
                                           "image of entry 0"):
        rd.Radler(s, psf, residual, residual, L.BEAM)
    with pytest.raises(RuntimeError, match=r"residual image of entry 0 is 64 x 47 pixels, the "
                                           r"settings give 64 x 48"):
        rd.Radler(s, small, small, rd.gpu.to_device(np.zeros((L.HEIGHT - 1, L.WIDTH),
                                                             np.float32)), L.BEAM)
    flat = rd.gpu.to_device(np.zeros(L.HEIGHT * L.WIDTH, np.float32))
    with pytest.raises(RuntimeError, match="2 or 3 dimensions"):
        rd.Radler(s, flat, flat.view(0, flat.shape), flat.view(0, flat.shape), L.BEAM)
    entry = rd.WorkTableEntry()
    with pytest.raises(RuntimeError, match=r"'model' has shape \(3072\), a 2-D"):
        entry.model = flat

    class Float64(L.CountingProducer):
        def __dlpack__(self, stream=None):
            capsule = super().__dlpack__(stream)
            list(L.CountingProducer.live.values())[-1][0].dl_tensor.dtype.bits = 64
            return capsule

    with pytest.raises(TypeError, match=r"'residual' has dtype \(code 2, 64 bits\), float32"):
        rd.Radler(s, psf, Float64(residual), model, L.BEAM)
    L.CountingProducer.live.clear()
    # nothing above consumed or changed the images
    assert rd.Radler(s, psf, residual, model, L.BEAM).perform(1) in (True, False)


def test_to_device_numpy_and_view():
    a = np.arange(5 * 7, dtype=np.float32).reshape(5, 7) - 3.0
    d = rd.gpu.to_device(a)
    assert d.shape == (5, 7) and d.dtype == "float32" and d.data_ptr % 16 == 0
    assert d.__dlpack_device__()[0] == 10
    assert np.array_equal(L.bits(d.numpy()), L.bits(a))
    v = d.view(8, (2, 7))
    assert v.data_ptr == d.data_ptr + 32 and np.array_equal(v.numpy(), a.ravel()[8:22].reshape(2, 7))
    with pytest.raises(RuntimeError, match="do not fit"):
        d.view(30, (6,))
    with pytest.raises(TypeError):
        rd.gpu.to_device(a.astype(np.float64))
    assert rd.gpu.to_device(np.zeros((0, 4), np.float32)).numpy().shape == (0, 4)


def test_cxx_host_over_device_accessors(tmp_path):
    from test_device_images import build_cxx_host
    host = subprocess.run([build_cxx_host(tmp_path), "gpu"], capture_output=True, text=True)
    assert host.returncode == 0 and host.stdout.strip() == "OK", host.stdout + host.stderr


# ------------------------------------------------------------- torch tensors
@pytest.fixture(scope="module")
def torch_results(tmp_path_factory):
    """Every torch case, run once in one child process."""
    results = tmp_path_factory.mktemp("device_images_torch") / "results.json"
    child = subprocess.run(
        [sys.executable, os.path.join(HERE, "device_images_torch_child.py"), str(results)],
        capture_output=True, text=True)
    report = f"exit status {child.returncode}\n{child.stdout[-2000:]}\n{child.stderr[-4000:]}"
    assert results.exists(), report
    return json.loads(results.read_text()), report


@pytest.mark.parametrize("case", TORCH_CASES)
def test_with_torch(torch_results, case):
    results, report = torch_results
    assert "child" not in results, results.get("child", "") + report
    assert case in results, report
    assert results[case] is None, results[case]
