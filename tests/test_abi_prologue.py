"""The opening every hope_env_* entry point shares (hope_amd/csrc/hope_handle.h): a NULL handle, and a pointer that hope_env_create
never returned, are refused before anything reads the handle -- and before any HIP call, so this needs no device.  Driven through the
prototype table of hope_amd/_lib.py: every exported hope_env_* function whose first parameter is the handle, all other arguments zero."""
import ctypes as C

import pytest

from hope_amd import _lib as L

EINVAL = -1
GETTERS = {'hope_env_num_scenes': EINVAL, 'hope_env_max_obstacles': EINVAL, 'hope_env_device_arch': b''}   # their "no handle" returns


def _handle_entries():
    lib = L.load_library()
    names = [n for n in L.EXPORTS if n.startswith('hope_env_') and n != 'hope_env_create']
    for n in names:
        at = getattr(lib, n).argtypes
        assert at and at[0] is C.c_void_p, f'{n}: no prototype in hope_amd/_lib.py, or its first parameter is not the handle'
    return names


ENTRIES = _handle_entries()


def _zero(argtype):
    if argtype in (C.c_void_p, C.c_char_p) or issubclass(argtype, C._Pointer):
        return None
    return argtype(0)


def _call(name, handle):
    lib = L.load_library()
    assert lib.hope_env_create(None, 0, 0, 0, 0) == EINVAL    # (no device touched) hope_last_error() now names another function
    fn = getattr(lib, name)
    return fn(handle, *[_zero(t) for t in fn.argtypes[1:]])


def _err():
    return L.load_library().hope_last_error().decode(errors='replace')


def test_the_table_covers_the_handle_entry_points():
    assert len(ENTRIES) >= 64 and 'hope_env_step' in ENTRIES and 'hope_env_set_pool' in ENTRIES and 'hope_env_eval_track' in ENTRIES


@pytest.mark.parametrize('name', ENTRIES)
def test_null_handle(name):
    rc = _call(name, None)
    if name == 'hope_env_destroy':
        assert rc == 0
    elif name in GETTERS:
        assert rc == GETTERS[name]
    else:
        assert rc == EINVAL and _err().startswith(name + ':'), (rc, _err())


@pytest.mark.parametrize('name', ENTRIES)
def test_pointer_that_was_never_a_handle(name):
    buf = C.create_string_buffer(64 * 1024)                   # zero-filled host memory, never returned by hope_env_create
    rc = _call(name, C.cast(buf, C.c_void_p))
    assert rc == GETTERS.get(name, EINVAL) and 'not a live handle' in _err(), (rc, _err())
    assert buf.raw == bytes(64 * 1024)                        # and nothing wrote to it
