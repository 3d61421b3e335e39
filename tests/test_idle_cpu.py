"""The free-voice query (skred_bank_find_idle / _find_idle_host) as far as a machine without a GPU can see it: the library exports
both entry points, the binding has both methods, and the argument checks come before anything touches the device."""
import ctypes as C

from skred_amd import device

BAD_ARG = -2


def test_library_exports_both_symbols():
    L = device.load()
    for s in ("skred_bank_find_idle", "skred_bank_find_idle_host"):
        assert hasattr(L, s), f"libskred_amd.so does not export {s}"
        assert s in device.ABI_SYMBOLS


def test_null_bank_and_null_query_are_bad_arguments():
    L = device.load()
    q = device.IdleQueryC(0, 1, device.IDLE_FINISHED, 0.0, 0, 0)
    cnt = (C.c_uint32 * 2)()
    total = C.c_int(0)
    assert L.skred_bank_find_idle(None, C.byref(q), None, cnt, None) == BAD_ARG
    assert L.skred_amd_last_error()
    assert L.skred_bank_find_idle_host(None, C.byref(q), None, C.byref(total), None) == BAD_ARG
    # a NULL query: the bank pointer is never followed (any non-NULL value will do)
    fake = C.c_void_p(C.addressof(cnt))
    assert L.skred_bank_find_idle(fake, None, None, cnt, None) == BAD_ARG
    assert L.skred_bank_find_idle_host(fake, None, None, C.byref(total), None) == BAD_ARG


def test_binding_has_both_methods_and_the_bits():
    assert callable(device.DeviceBank.find_idle) and callable(device.DeviceBank.find_idle_host)
    assert (device.IDLE_FINISHED, device.IDLE_ENV_DONE, device.IDLE_AMP_ZERO, device.IDLE_UNNAMED) == (1, 2, 4, 256)
    assert C.sizeof(device.IdleQueryC) == 24
