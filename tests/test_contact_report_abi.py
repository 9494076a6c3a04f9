"""Contact reports without a device: the record layouts against include/xpbd.h, the exported symbols, argument errors on a
NULL world, the model's event order, and a world that cannot be created without a device."""
import ctypes as C
import os
import re

import numpy as np

import contact_report_model as rm
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["xpbd_world_set_contact_report", "xpbd_world_contact_report_counts", "xpbd_world_download_pair_contacts",
               "xpbd_world_download_contact_events", "xpbd_multi_world_set_contact_report", "xpbd_multi_world_contact_report_counts",
               "xpbd_multi_world_download_pair_contacts", "xpbd_multi_world_download_contact_events"]


def header_fields(name):
    header = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, names in re.findall(r"(uint32_t|double)\s+([^;]+);", body):
        for field in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?", field)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


def check_dtype(dt, name, size):
    assert dt.itemsize == size
    offset = 0
    for field, ctype, count in header_fields(name):
        width = 4 if ctype == "uint32_t" else 8
        offset = (offset + width - 1) // width * width
        assert dt.fields[field][1] == offset, (name, field)
        assert dt.fields[field][0].itemsize == width * count, (name, field)
        offset += width * count
    assert offset == size
    assert [f for f, _, _ in header_fields(name)] == list(dt.names)


def test_record_layouts_match_the_header():
    check_dtype(capi.PAIR_CONTACT_DTYPE, "xpbd_pair_contact", 64)
    check_dtype(capi.CONTACT_POINT_DTYPE, "xpbd_contact_point", 48)
    check_dtype(capi.CONTACT_EVENT_DTYPE, "xpbd_contact_event", 12)
    header = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    assert re.search(r"#define XPBD_CONTACT_BEGIN 0u", header) and re.search(r"#define XPBD_CONTACT_END\s+1u", header)
    assert (capi.CONTACT_BEGIN, capi.CONTACT_END) == (0, 1)


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    counts = (C.c_uint32 * 4)()
    n, m = C.c_uint32(7), C.c_uint32(7)
    pairs = np.zeros(2, dtype=capi.PAIR_CONTACT_DTYPE)
    events = np.zeros(2, dtype=capi.CONTACT_EVENT_DTYPE)
    for enable in (0, 1, 2):
        assert L.xpbd_world_set_contact_report(None, enable) == capi.E_INVALID
        assert b"NULL world" in L.xpbd_last_error()
    assert L.xpbd_world_contact_report_counts(None, counts) == capi.E_INVALID
    assert L.xpbd_world_download_pair_contacts(None, pairs.ctypes.data, 2, None, 0, C.byref(n), C.byref(m)) == capi.E_INVALID
    assert L.xpbd_world_download_pair_contacts(None, None, 0, None, 0, None, None) == capi.E_INVALID
    assert L.xpbd_world_download_contact_events(None, events.ctypes.data, 2, C.byref(n)) == capi.E_INVALID
    assert L.xpbd_world_download_contact_events(None, None, 0, None) == capi.E_INVALID
    for enable in (0, 1, 2):
        assert L.xpbd_multi_world_set_contact_report(None, enable) == capi.E_INVALID
        assert b"NULL world" in L.xpbd_last_error()
    assert L.xpbd_multi_world_contact_report_counts(None, counts) == capi.E_INVALID
    assert L.xpbd_multi_world_download_pair_contacts(None, pairs.ctypes.data, 2, None, 0, C.byref(n), C.byref(m)) == capi.E_INVALID
    assert L.xpbd_multi_world_download_pair_contacts(None, None, 0, None, 0, None, None) == capi.E_INVALID
    assert L.xpbd_multi_world_download_contact_events(None, events.ctypes.data, 2, C.byref(n)) == capi.E_INVALID
    assert (n.value, m.value) == (7, 7)                      # nothing is written on an argument error


def test_no_device_fails_like_every_other_call():
    """Without a usable device a world cannot be created, so no report call can run (no CPU fallback); with one this is moot."""
    L = capi.hip_lib()
    if L.xpbd_device_count() > 0:
        return
    cfg = capi.Config()
    L.xpbd_config_default(C.byref(cfg))
    cfg.mode = capi.MODE_CONTACTS
    h = C.c_void_p()
    rc = L.xpbd_world_create(C.byref(h), C.byref(cfg))
    assert rc in (capi.E_NO_DEVICE, capi.E_HIP) and not h.value
    assert L.xpbd_world_set_contact_report(h, 1) == capi.E_INVALID


def test_model_events_are_begins_then_ends_in_key_order():
    prev = [(0, 1), (0, 5), (2, 3), (4, 9)]
    cur = [(0, 2), (0, 5), (1, 2), (4, 9), (7, 8)]
    ev = rm.events(prev, cur)
    assert ev == [(0, 2, capi.CONTACT_BEGIN), (1, 2, capi.CONTACT_BEGIN), (7, 8, capi.CONTACT_BEGIN),
                  (0, 1, capi.CONTACT_END), (2, 3, capi.CONTACT_END)]
    assert rm.events([], cur) == [(a, b, capi.CONTACT_BEGIN) for a, b in cur]
    assert rm.events(cur, cur) == []
    off = np.array([0, 2, 4, 5, 6], dtype=np.uint32)        # the pair list the tests derive from CSR neighbour lists
    nb = np.array([1, 3, 0, 2, 1, 0], dtype=np.uint32)
    assert rm.upper_pairs(off, nb) == [(0, 1), (0, 3), (1, 2)]

