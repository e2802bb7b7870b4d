"""What the six owners of a native handle share (viettts_amd/_handle.py) and the one blob rule behind every pack() / bind_packed()
(vtts_internal.h: check_blob), without a GPU: constructing an owner on "cuda:0" only builds host-side tables."""
import ctypes as C

import pytest

from viettts_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _generator(device):
    from viettts_amd.hifigan.generator import Generator

    return Generator(device=device)


def _duration(device):
    from viettts_amd.nat.duration import DurationModel

    return DurationModel(device=device)


def _acoustic(device):
    from viettts_amd.nat.acoustic import AcousticModel

    return AcousticModel(device=device)


def _mel(device):
    from viettts_amd.nat.dsp import MelFilter

    return MelFilter(16000, 1024, 80, 0.0, 8000, device=device)


def _disc(device):
    from viettts_amd.hifigan.discriminators import Discriminators

    return Discriminators(device)


def _audio(device):
    from viettts_amd.audio import Resampler

    return Resampler(16000, 44100, device)


# (C prefix, owner on a device, entries of param_table() or None where the handle takes no checkpoint arrays)
OWNERS = [("vtts_hifigan", _generator, 156), ("vtts_nat_duration", _duration, 27), ("vtts_nat_acoustic", _acoustic, 57), ("vtts_mel", _mel, None),
          ("vtts_disc", _disc, 108), ("vtts_audio", _audio, None)]
IDS = [o[0] for o in OWNERS]


@pytest.mark.parametrize("prefix, make, n_params", OWNERS, ids=IDS)
def test_owner_lifetime_and_device_rule(lib, prefix, make, n_params):
    with pytest.raises(ValueError):
        make("cpu")
    o = make("cuda:0")
    assert o.device.type == "cuda" and o.device.index == 0 and o._h.value and o.lib is lib
    assert o.packed_bytes > 0 and o.packed_bytes % 4 == 0
    if n_params is not None:
        table = o.param_table()
        assert len(table) == n_params and all(len(shape) >= 1 and min(shape) >= 1 for _, _, shape in table)
    with pytest.raises(RuntimeError):
        o.packed_blob()  # nothing loaded
    o.close()
    assert not o._h.value and o._blob is None and o._ws is None
    o.close()  # twice is harmless
    with pytest.raises(_lib.VttsError) as e:
        o.packed_bytes
    assert e.value.status == -1
    o.__del__()


def test_a_constructor_that_fails_leaves_an_object_that_closes(lib):
    from viettts_amd.audio import Resampler

    for args, exc in (((0, 16000, "cuda:0"), _lib.VttsError), ((16000, 8000, "cpu"), ValueError)):
        o = Resampler.__new__(Resampler)
        with pytest.raises(exc):
            o.__init__(*args)
        assert not o._h.value
        o.close()  # what __del__ runs: no handle to destroy, nothing raised
        o.__del__()
    Resampler.__new__(Resampler).close()  # not even __init__'s first line ran


@pytest.mark.parametrize("prefix, make, n_params", OWNERS, ids=IDS)
def test_one_blob_rule_for_every_handle(lib, prefix, make, n_params):
    """bind_packed() / pack() straight on the C functions with addresses that are never dereferenced: every call is refused, or only
    recorded, on the host."""
    o = make("cuda:0")
    bind, pack = getattr(lib, prefix + "_bind_packed"), getattr(lib, prefix + "_pack")
    need, base = o.packed_bytes, 1 << 32
    assert bind(o._h, C.c_void_p(base), need - 4) == -5 and b"too small" in lib.vtts_last_error()
    assert bind(o._h, C.c_void_p(base | 64), need) == -1 and b"aligned" in lib.vtts_last_error()  # aligned to 64 only: the kernels read float4 / uint4
    assert bind(o._h, None, need) == -1 and b"null" in lib.vtts_last_error()
    assert bind(o._h, C.c_void_p(base), need) == 0
    assert bind(o._h, C.c_void_p(base), need + 256) == 0  # a larger blob (a caller's own rounding) is fine
    assert pack(o._h, None, need, None) == -1 and b"null" in lib.vtts_last_error()
    assert pack(o._h, C.c_void_p(base), need - 4, None) == -5
    assert pack(o._h, C.c_void_p(base | 64), need, None) == -1 and b"aligned" in lib.vtts_last_error()
    o.close()


def test_every_export_has_a_prototype(lib):
    groups = (_lib.EXPORTS, _lib.NAT_EXPORTS, _lib.MEL_EXPORTS, _lib.DISC_EXPORTS, _lib.AUDIO_EXPORTS)
    listed = [name for g in groups for name in g]
    assert len(listed) == len(set(listed)) and set(listed) == set(_lib.SIGS)  # each symbol in exactly one header's list
    assert {"vtts_abi_version", "vtts_last_error"} <= set(_lib.EXPORTS)
    for name, (res, args) in _lib.SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
