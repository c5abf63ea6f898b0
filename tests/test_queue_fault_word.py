"""The cross-XCC queue's sticky fault word, host side (crc32c_engine.cc).

A wave of the fixed kernel's work queue that runs into its spin cap drops its
groups and sets a word in pinned host memory held in the device's state; from
then on every engine call on that device fails with LSBM_ERR_QUEUE_FAULT.  Here
the word is set by the test hook (no kernel runs, no device is needed): the
device ordinal used is one no machine has, so a clear word gives
LSBM_ERR_NO_DEVICE."""
from lsbm_amd import _lib

DEV = 63  # (kMaxDevices - 1: never a real device)


def test_fault_word_is_sticky_and_per_device(product_lib):
    L = product_lib
    assert L.lsbm_crc32c_init(DEV) == _lib.LSBM_ERR_NO_DEVICE
    assert L.lsbm_test_queue_fault(DEV, 1) == 0  # (was clear)
    try:
        for _ in range(3):  # every later call
            assert L.lsbm_crc32c_init(DEV) == _lib.LSBM_ERR_QUEUE_FAULT
            assert b"spin cap" in L.lsbm_crc32c_last_error()
        assert L.lsbm_crc32c_init(DEV - 1) == _lib.LSBM_ERR_NO_DEVICE  # another device's word
    finally:
        assert L.lsbm_test_queue_fault(DEV, 0) == 1  # (was set)
    assert L.lsbm_crc32c_init(DEV) == _lib.LSBM_ERR_NO_DEVICE


def test_hook_arguments(product_lib):
    L = product_lib
    assert L.lsbm_test_queue_fault(-1, 1) == -1
    assert L.lsbm_test_queue_fault(64, 1) == -1
    assert L.lsbm_test_queue_fault(DEV, 2) == -1
    assert L.lsbm_test_fixed_queue(3) == -1
    assert L.lsbm_test_fixed_tail(0, 1) == -1
    assert L.lsbm_test_fixed_tail(2, 0) == -1
    for mode in (0, 1, 2, -1):
        assert L.lsbm_test_fixed_queue(mode) == 0
    assert L.lsbm_test_fixed_tail(2, 1) == 0
    assert L.lsbm_test_fixed_tail(-1, -1) == 0
    assert L.lsbm_test_queue_pool(2) == -1
    assert L.lsbm_test_queue_pool(1) == 0
    assert L.lsbm_test_queue_pool_busy(63) == -1  # (no such device: no pool)
