"""Shared by tests/test_device_images_gpu.py and its torch child: the problems,
and the comparison of a Radler over numpy arrays with one over the same data
in device memory.

A backend says how device images are made and read: radler's own
(radler.gpu.to_device / DeviceArray) here, torch's in the child.
"""
import ctypes as C

import numpy as np

from radler_import import radler as rd
from synthetic import problem

WIDTH, HEIGHT = 64, 48
PIXEL_SCALE = 1.0 / 60.0 * np.pi / 180.0
BEAM = 0.0
ALL = ("psf", "residual", "model")
BANDS = [(100e6 + 10e6 * i, 110e6 + 10e6 * i) for i in range(4)]
WEIGHTS = [1.0, 0.0, 2.5, 0.75]          # unequal, one of them 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class RadlerBackend:
    """radler.gpu.DeviceArray"""

    @staticmethod
    def to_device(array):
        return rd.gpu.to_device(np.ascontiguousarray(array, np.float32))

    @staticmethod
    def to_host(device_array):
        return device_array.numpy()

    @staticmethod
    def pointer(device_array):
        return device_array.data_ptr

    @staticmethod
    def plane(device_array, index):
        height, width = device_array.shape[-2:]
        return device_array.view(index * height * width, (height, width))


def inputs(n_images, width=WIDTH, height=HEIGHT, seed=11, points=12):
    """psf, residual, model of shape (n_images, height, width): one sky per
    image (brighter with the index), each with a PSF of its own width."""
    psfs, residuals = [], []
    for i in range(n_images):
        psf, dirty = problem(width, height, n_points=points, n_blobs=1, seed=seed,
                             fwhm=3.0 + 0.4 * i)
        psfs.append(psf.astype(np.float32))
        residuals.append((dirty * (1.0 + 0.15 * i)).astype(np.float32))
    psf, residual = np.stack(psfs), np.stack(residuals)
    return psf, residual, np.zeros_like(residual)


def settings(width=WIDTH, height=HEIGHT, algorithm=None):
    s = rd.Settings()
    s.algorithm_type = algorithm or rd.AlgorithmType.generic_clean
    s.trimmed_image_width, s.trimmed_image_height = width, height
    s.pixel_scale.x = s.pixel_scale.y = PIXEL_SCALE
    s.minor_iteration_count = 120
    s.absolute_threshold = 4e-3
    s.major_loop_gain = 0.6                # perform(2) has work left
    return s


def components(radler):
    cl = radler.component_list
    out = []
    for scale in range(cl.n_scales):
        positions = cl.get_positions(scale)
        values = [cl.get_component(scale, i) for i in range(cl.component_count(scale))]
        out.append((positions, values))
    return out


def compare(build, psf, residual, model, backend=RadlerBackend, device=ALL, make_device=None):
    """build(psf, residual, model) -> Radler, called on copies of the numpy
    arrays and on the same data with the arguments named in `device` in device
    memory (make_device(name, array) when given, else backend.to_device).
    perform(1) and perform(2) on both: the same flag and iteration number, the
    same bits in residual and model, an untouched PSF, device images still at
    their addresses; then the same component list. Returns both Radlers and
    the device-side arguments."""
    originals = dict(psf=psf, residual=residual, model=model)
    host = {k: v.copy() for k, v in originals.items()}
    mixed = {}
    for k, v in originals.items():
        if k not in device:
            mixed[k] = v.copy()
        else:
            mixed[k] = make_device(k, v) if make_device else backend.to_device(v)
    pointers = {k: backend.pointer(mixed[k]) for k in device}
    of_host, of_device = build(**host), build(**mixed)

    def read(k):
        return backend.to_host(mixed[k]) if k in device else mixed[k]

    for major in (1, 2):
        flag_host, flag_device = of_host.perform(major), of_device.perform(major)
        assert flag_host == flag_device, major
        assert of_host.iteration_number == of_device.iteration_number, major
        for k in ("residual", "model"):
            got = read(k)
            assert got.shape == host[k].shape
            assert np.array_equal(bits(got), bits(host[k])), (k, major)
        assert np.array_equal(bits(host["psf"]), bits(psf))
        assert np.array_equal(bits(read("psf")), bits(psf)), major
        for k in device:
            assert backend.pointer(mixed[k]) == pointers[k], (k, major)
    assert of_host.iteration_number > 0 and np.any(host["model"] != 0)
    assert not np.array_equal(bits(host["residual"]), bits(residual))
    assert components(of_host) == components(of_device)
    return of_host, of_device, mixed


def simple(s, **keywords):
    return lambda psf, residual, model: rd.Radler(s, psf, residual, model, BEAM, **keywords)


def channels_case(fitting=None, terms=2):
    """Four channels with WEIGHTS (channel 1: weight 0, a residual of NaNs) in
    two deconvolution groups. Returns (build, psf, residual, model)."""
    psf, residual, model = inputs(4)
    residual[1] = np.nan
    s = settings()
    if fitting is not None:
        s.spectral_fitting.mode = fitting
        s.spectral_fitting.terms = terms
    return simple(s, n_deconvolution_groups=2, frequencies=np.array(BANDS),
                  weights=np.array(WEIGHTS)), psf, residual, model


def polarizations_case(backend=RadlerBackend):
    """One channel, Stokes I and Q linked, built entry by entry. The arrays are
    (2, height, width): plane p is polarization p; one PSF."""
    psf, residual, model = inputs(2)
    psf = psf[:1]
    residual[1] *= -0.4
    s = settings()
    s.linked_polarizations = {rd.Polarization.stokes_i, rd.Polarization.stokes_q}

    def plane(stack, index):
        return stack[index] if isinstance(stack, np.ndarray) else backend.plane(stack, index)

    def build(psf, residual, model):
        table = rd.WorkTable([], 1, 1)
        for p, polarization in enumerate([rd.Polarization.stokes_i, rd.Polarization.stokes_q]):
            e = rd.WorkTableEntry()
            e.polarization = polarization
            e.band_start_frequency, e.band_end_frequency = BANDS[0]
            e.image_weight = 1.0
            if p == 0:
                e.psfs.append(plane(psf, 0))
            e.residual = plane(residual, p)
            e.model = plane(model, p)
            table.add_entry(e)
        return rd.Radler(s, table, BEAM)
    return build, psf, residual, model


def multiscale_grid_case():
    size = 128
    psf, residual, model = inputs(1, size, size, seed=3, points=30)
    s = settings(size, size, rd.AlgorithmType.multiscale)
    s.multiscale.max_scales = 3
    s.save_source_list = True
    s.parallel.grid_width = s.parallel.grid_height = 2
    s.parallel.max_threads = 2
    return simple(s), psf[0], residual[0], model[0]


# ------------------------------------------------- a DLPack producer of our own
class _DLDevice(C.Structure):
    _fields_ = [("device_type", C.c_int32), ("device_id", C.c_int32)]


class _DLDataType(C.Structure):
    _fields_ = [("code", C.c_uint8), ("bits", C.c_uint8), ("lanes", C.c_uint16)]


class _DLTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("device", _DLDevice), ("ndim", C.c_int32),
                ("dtype", _DLDataType), ("shape", C.POINTER(C.c_int64)),
                ("strides", C.POINTER(C.c_int64)), ("byte_offset", C.c_uint64)]


class _DLManagedTensor(C.Structure):
    pass


_DELETER = C.CFUNCTYPE(None, C.POINTER(_DLManagedTensor))
_DLManagedTensor._fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", C.c_void_p),
                             ("deleter", _DELETER)]
_CAPSULE_NAME = b"dltensor"
_new_capsule = C.pythonapi.PyCapsule_New
_new_capsule.restype = C.py_object
_new_capsule.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]


class CountingProducer:
    """A DLPack producer over a DeviceArray's memory whose tensors are its own
    (DLManagedTensor structs made here), so that it sees their deleters run:
    `exported` capsules handed out, `deleted` deleter calls. A live tensor
    holds the DeviceArray (the memory) whether or not the producer is still
    referenced, as the protocol requires. `shape` / `byte_offset` export a
    view that starts byte_offset bytes into the array."""
    live, dead = {}, []

    def __init__(self, array, shape=None, byte_offset=0, counts=None):
        self.array, self.shape, self.byte_offset = array, tuple(shape or array.shape), byte_offset
        self.counts = counts if counts is not None else dict(exported=0, deleted=0)

    def __dlpack_device__(self):
        return self.array.__dlpack_device__()

    def __dlpack__(self, stream=None):
        counts = self.counts
        managed = _DLManagedTensor()
        shape = (C.c_int64 * len(self.shape))(*self.shape)
        key = C.addressof(managed)

        def deleter(pointer):
            # gives the memory back; the struct and this very callback stay
            # allocated (it is still running)
            counts["deleted"] += 1
            entry = CountingProducer.live.pop(key)
            entry[3] = None
            CountingProducer.dead.append(entry)

        callback = _DELETER(deleter)
        t = managed.dl_tensor
        t.data, t.byte_offset = self.array.data_ptr, self.byte_offset
        t.device = _DLDevice(*self.array.__dlpack_device__())
        t.ndim, t.dtype = len(self.shape), _DLDataType(2, 32, 1)
        t.shape = C.cast(shape, C.POINTER(C.c_int64))
        t.strides = None
        managed.manager_ctx, managed.deleter = None, callback
        CountingProducer.live[key] = [managed, shape, callback, self.array]
        counts["exported"] += 1
        return _new_capsule(key, _CAPSULE_NAME, None)
