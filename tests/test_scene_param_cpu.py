"""param_layout (jur_param_layout): the layout of the parameter-error entry, host arithmetic with no GPU.  The widths wb_s
of the parameter blocks per slice and the running sums bwptr, cptr and bbptr against a direct count in numpy on seeded
ragged layouts; every layout refusal by its words; the new symbols and the sizes of the two structs."""
import ctypes as C
import numpy as np
import pytest


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    return lib


def layout(rng, nslice, nr, widths=(0, 1, 3, 7, 64, 65), lead=True):
    """sid with the rays of the slices interleaved (and one leading ray without a slice), w_s and wb_s drawn from widths"""
    w = rng.choice([x for x in widths if x > 0], nslice)
    wb = rng.choice(widths, nslice)
    sid = rng.integers(-1, nslice, nr).astype(np.int32)
    if lead and nr:
        sid[0] = -1
    wr = np.where(sid >= 0, w[np.maximum(sid, 0)], 0)
    # a ray without a slice may have any width in rowptr_b: it is not looked at
    wbr = np.where(sid >= 0, wb[np.maximum(sid, 0)], rng.integers(0, 5, nr))
    used = np.isin(np.arange(nslice), sid)
    wptr = np.concatenate([[0], np.cumsum(w)]).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(wr)]).astype(np.int64)
    rowptr_b = np.concatenate([[0], np.cumsum(wbr)]).astype(np.int64)
    return wptr, rowptr, rowptr_b, sid, w, np.where(used, wb, 0)


def running(a):
    return np.concatenate([[0], np.cumsum(a)]).astype(np.int64)


def test_against_a_count(hip):
    rng = np.random.default_rng(17)
    met_zero = met_unused = 0
    for trial in range(200):
        nslice, nr = int(rng.integers(1, 8)), int(rng.integers(0, 41))
        wptr, rowptr, rowptr_b, sid, w, wb = layout(rng, nslice, nr)
        got = hip.param_layout(wptr, rowptr, rowptr_b, sid)
        assert np.array_equal(got["bwptr"], running(wb)), trial
        assert np.array_equal(got["cptr"], running(w * wb)), trial
        assert np.array_equal(got["bbptr"], running(wb * wb)), trial
        met_zero += int(np.any((wb == 0) & np.isin(np.arange(nslice), sid)))
        met_unused += int(not np.all(np.isin(np.arange(nslice), sid)))
    assert met_zero > 10 and met_unused > 10                        # slices with wb = 0, slices without rays


def test_named_cases(hip):
    # a leading ray without a slice, a slice with wb = 0, the rays of two slices interleaved
    wptr = np.array([0, 3, 5, 9])
    sid = np.array([-1, 0, 2, 0, 1, 2, 0], dtype=np.int32)
    w, wb = np.array([3, 2, 4]), np.array([6, 0, 65])
    rowptr = running(np.where(sid >= 0, w[sid], 0))
    rowptr_b = running(np.where(sid >= 0, wb[sid], 2))
    got = hip.param_layout(wptr, rowptr, rowptr_b, sid)
    assert list(got["bwptr"]) == [0, 6, 6, 71]
    assert list(got["cptr"]) == [0, 18, 18, 18 + 260]
    assert list(got["bbptr"]) == [0, 36, 36, 36 + 65 * 65]


def raw(hip, wptr, rowptr, rowptr_b, sid, outs=(None, None, None)):
    lp_, ip_ = C.POINTER(C.c_long), C.POINTER(C.c_int)
    a = [None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (wptr, rowptr, rowptr_b)]
    s = None if sid is None else np.ascontiguousarray(sid, dtype=np.int32)
    rc = hip.lib().jur_param_layout(len(wptr) - 1 if wptr is not None else 1, None if a[0] is None else a[0].ctypes.data_as(lp_),
                                    len(sid) if sid is not None else 1, None if a[1] is None else a[1].ctypes.data_as(lp_),
                                    None if a[2] is None else a[2].ctypes.data_as(lp_), None if s is None else s.ctypes.data_as(ip_),
                                    *[None if o is None else o.ctypes.data_as(lp_) for o in outs])
    return rc, hip.lib().jur_last_error().decode()


def test_null_outputs_count_only(hip):
    rng = np.random.default_rng(3)
    wptr, rowptr, rowptr_b, sid, w, wb = layout(rng, 5, 30)
    rc, _ = raw(hip, wptr, rowptr, rowptr_b, sid)
    assert rc == int((w * wb).sum())
    only = np.full(6, -7, dtype=np.int64)
    rc2, _ = raw(hip, wptr, rowptr, rowptr_b, sid, outs=(None, only, None))
    assert rc2 == rc and np.array_equal(only, running(w * wb))
    rc0, _ = raw(hip, np.array([0]), np.array([0]), np.array([0]), np.zeros(0, np.int32))
    assert rc0 == 0


def test_refusals(hip):
    wptr = np.array([0, 3, 5])
    sid = np.array([-1, 0, 1, 0], dtype=np.int32)
    rowptr, rowptr_b = np.array([0, 0, 3, 5, 8]), np.array([0, 1, 5, 7, 11])
    sent = [np.full(3, -7, dtype=np.int64) for _ in range(3)]

    def refused(words, **kw):
        args = dict(wptr=wptr, rowptr=rowptr, rowptr_b=rowptr_b, sid=sid)
        args.update(kw)
        rc, msg = raw(hip, args["wptr"], args["rowptr"], args["rowptr_b"], args["sid"], outs=sent)
        assert rc == hip.EINVAL and msg == "jur_param_layout: " + words, msg
        assert all(np.all(o == -7) for o in sent), "outputs of a refused call were written"

    assert raw(hip, wptr, rowptr, rowptr_b, sid)[0] == 3 * 4 + 2 * 2
    refused("wptr is not an ascending running sum of widths from 0 (slice 1)", wptr=np.array([0, 3, 2]))
    refused("wptr is not an ascending running sum of widths from 0 (slice 0)", wptr=np.array([1, 3, 5]))
    refused("sid of ray 2 is 2: outside -1..1", sid=np.array([-1, 0, 2, 0], dtype=np.int32))
    refused("the block of ray 2 has 3 columns, its slice 1 has 2 elements", rowptr=np.array([0, 0, 3, 6, 9]))
    refused("the block of ray 0 has 1 columns, its slice -1 has 0 elements", rowptr=np.array([0, 1, 4, 6, 9]))
    refused("rowptr does not start at 0", rowptr=rowptr + 1)
    refused("rowptr_b does not start at 0", rowptr_b=rowptr_b + 1)
    refused("rowptr_b is not ascending at ray 2", rowptr_b=np.array([0, 1, 5, 4, 8]))
    refused("rays 1 and 3 of slice 0 have 4 and 5 columns in rowptr_b", rowptr_b=np.array([0, 1, 5, 7, 12]))
    refused("null argument", rowptr_b=None)
    refused("null argument", wptr=None)
    with pytest.raises(hip.JurassicError, match=r"error %d: jur_param_layout: rays 1 and 3 of slice 0 have 4 and 5 columns" % hip.EINVAL):
        hip.param_layout(wptr, rowptr, np.array([0, 1, 5, 7, 12]), sid)
    with pytest.raises(ValueError):
        hip.param_layout(wptr, rowptr, rowptr_b[:-1], sid)


def test_abi(hip):
    L = hip.lib()
    for name in ("jur_param_slices_host", "jur_param_layout", "jur_param_abi_sizes", "jur_model_set_ret_windows",
                 "jur_model_ret_windows"):
        assert hasattr(L, name), name
    out = (C.c_size_t * 2)()
    L.jur_param_abi_sizes(out)
    assert list(out) == [C.sizeof(hip.ParamIn), C.sizeof(hip.ParamOut)] == [24, 16]
    assert hip.ParamIn.var.offset == 8 and hip.ParamIn.cov.offset == 16 and hip.ParamIn.ncov.offset == 4
    assert hip.ParamOut.C.offset == 0 and hip.ParamOut.sigma_param.offset == 8
    # no model: the setter and the getter refuse a NULL by their words and touch nothing
    from jurassic_hip import abi
    ctl = abi.ctl_t()
    assert L.jur_model_set_ret_windows(None, C.byref(ctl)) == hip.EINVAL
    assert "jur_model_set_ret_windows: null argument" in L.jur_last_error().decode()
    assert L.jur_model_ret_windows(None, C.byref(ctl)) == hip.EINVAL
    assert "jur_model_ret_windows: null argument" in L.jur_last_error().decode()
