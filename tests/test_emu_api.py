"""The wave emulator's interface (tests/emu/emu_api.h, tests/emu_py.py): the ctypes mirrors of its argument blocks, settings that
hold for one call and no longer, and the model family the launcher and the emulator both pick (csrc/step_plan.h: ck::pick_family)."""
import ctypes

import numpy as np
import pytest

import emu_py
from cassie_amd import Model
from cassie_amd._lib import CmModel

CASSIE, CASSIE_HFIELD, CASSIE_ALL, TRAY, TRAY_HFIELD, GENERIC32, GENERIC40 = range(7)     # ck::StepFamily


def test_ctypes_mirrors_have_the_c_structs_sizes_and_offsets(built):
    L = emu_py.lib()
    for which, T in enumerate(emu_py.API):
        assert ctypes.sizeof(T) == L.emu_sizeof_api(which), T.__name__
        for k, (f, _) in enumerate(T._fields_):
            assert getattr(T, f).offset == L.emu_offsetof_api(which, k), (T.__name__, f)
        assert L.emu_offsetof_api(which, len(T._fields_)) == -1, T.__name__      # (the mirror has every field)
    assert L.emu_sizeof_api(len(emu_py.API)) == 0


def _run(cassie, **settings):
    emu = emu_py.EmuBatch(cassie.pod, 2)
    emu.qpos[:] = cassie.qpos_init()
    emu.qpos[1, 2] -= 0.05
    emu.ctrl[:] = [1.0, -2.0, 3.0, -4.0, 0.5, -1.0, 2.0, -3.0, 4.0, -0.5]
    emu.settings = settings
    emu.step(4)
    return [getattr(emu, f).tobytes() for f in ("qpos", "qvel", "qacc_warmstart", "qacc", "sensordata", "actuator_velocity", "time", "warn",
                                                 "info", "xpos", "xquat")]


OTHER = dict(fast_rows=1, two_waves=1, chunks=2, poison_lds=1, wave_schedule=2)


def test_settings_hold_for_one_call(cassie):
    a = _run(cassie)
    _run(cassie, **OTHER)
    assert _run(cassie) == a


def test_settings_block_left_by_an_exception_leaves_nothing(cassie):
    a = _run(cassie)
    with pytest.raises(RuntimeError):
        with emu_py.settings(**OTHER):
            _run(cassie)
            raise RuntimeError("inside the block")
    assert _run(cassie) == a


def test_family_of_the_shipped_models_and_of_edited_ones(built):
    pods = {name: Model(name).pod for name in ("cassie", "cassie_hfield", "cassie_tray_box")}
    assert [emu_py.pick_family(pods[n]) for n in ("cassie", "cassie_hfield", "cassie_tray_box")] == [CASSIE, CASSIE_HFIELD, TRAY]
    assert emu_py.pick_family(pods["cassie"], generic_only=True) == GENERIC32
    tray = CmModel.from_buffer_copy(pods["cassie_tray_box"])
    tray.hfield_geom = 0
    assert emu_py.pick_family(tray) == TRAY_HFIELD
    other = CmModel.from_buffer_copy(pods["cassie"])
    other.dof_ancmask[7] ^= 1
    assert emu_py.pick_family(other) == GENERIC32
