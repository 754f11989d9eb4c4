"""The S16 convolution's instance table (tests/s16_instances.py) is the library's, both ways — on the host, through
tcs_conv2d_s16_plan (plans, launches nothing, touches no tensor).  Whatever plans with TCS_OK is in the table and the table holds
nothing the library refuses, so an `S16_CASE` added to or removed from launch_s16_cfg fails here until the table — and with it the
GPU cases of test_gpu_s16_instances.py, which are parametrised from the same table — follows.  The heuristic is not restated: the
library is asked which instance it picks for the loop's layers."""
import ctypes as C

import pytest

import s16_instances as si


def _lib():
    from tcs_mi355 import native
    return native, native.lib()


# the sweep's layer per epilogue: 64 input channels = 4 k-steps (KSTEPS 1, 2 and 4 divide it), outputs that allow MT = 2
_SWEEP_COUT = {si.EPI_LINEAR: 128, si.EPI_GRU_ZR: 128, si.EPI_GRU_Q: 64, si.EPI_DECONV2X: 128, si.EPI_BLEND9: 9}
_H, _W = 13, 70


def test_plan_is_exported_and_abi_version():
    native, lib = _lib()
    assert lib.tcs_abi_version() >= 17
    assert C.sizeof(native.S16Instance) == 14 * 4 + 8
    assert lib.tcs_conv2d_s16_plan(None, None) == si.TCS_EINVAL
    d = si.host_desc(native, 3, 1, si.EPI_LINEAR, 0, (64,), 128, _H, _W)
    assert lib.tcs_conv2d_s16_plan(C.byref(d), None) == si.TCS_EINVAL
    # what tcs_conv2d_s16 refuses before its launch is refused with the same code
    d.Cin = 63
    assert si.plan(native, lib, d)[0] == si.TCS_EINVAL
    d = si.host_desc(native, 5, 1, si.EPI_LINEAR, 0, (64,), 128, _H, _W)
    assert si.plan(native, lib, d)[0] == si.TCS_EUNSUPPORTED
    d = si.host_desc(native, 3, 2, si.EPI_GRU_Q, 0, (64,), 64, _H, _W)
    assert si.plan(native, lib, d)[0] == si.TCS_EUNSUPPORTED


@pytest.mark.parametrize("products", (0, 1, 3))
@pytest.mark.parametrize("epilogue", sorted(si.EPI_NAME))
def test_codes_that_plan_equal_the_table(epilogue, products):
    """Every (ksize, stride, taps) of this epilogue, the whole code space, with and without a CSPLIT digit: the set that plans with
    TCS_OK equals the table's row (empty where there is none); the reported fields are the code's digits."""
    native, lib = _lib()
    cout = _SWEEP_COUT[epilogue]
    seen_kinds = 0
    for ksize in (1, 3):
        for stride in (1, 2):
            for taps in (0, 1):
                kind = (ksize, stride, epilogue, taps)
                ok = set()
                for code in si.code_space():
                    rcs = []
                    for csplit in (0, 1):
                        d = si.host_desc(native, ksize, stride, epilogue, taps, (64,), cout, _H, _W, B=3, products=products,
                                         tile_cfg=csplit * 100000 + code)
                        rc, p = si.plan(native, lib, d)
                        rcs.append(rc)
                        assert rc in (si.TCS_OK, si.TCS_EINVAL, si.TCS_EUNSUPPORTED), (kind, code, rc)
                        if rc != si.TCS_OK:
                            continue
                        rs, rpw, mt, rows, kst, nst = si.digits(code)
                        assert (p.ksize, p.stride, p.epilogue, p.taps) == kind, (kind, code)
                        assert (p.row_split, p.rows_per_wave, p.mt, p.rows, p.ksteps, p.nstage) == (rs, rpw, mt, rows, kst, nst), (kind, code)
                        assert p.products == (3 if products == 0 else products), (kind, code)
                        assert p.csplit == csplit, (kind, code)
                        assert p.threads == 64 * rows // rpw, (kind, code)
                        Ho, Wo = ((_H - 1) // 2 + 1, (_W - 1) // 2 + 1) if stride == 2 else (_H, _W)
                        assert p.blocks == -(-Wo // 32) * -(-Ho // rows) * (-(-cout // 32) // mt), (kind, code)
                        assert 0 < p.lds_bytes <= 160 * 1024 and p.lds_bytes % (1024 * nst) == 0, (kind, code)
                    assert rcs[0] == rcs[1], (kind, code, rcs)              # the CSPLIT digit never decides whether a code exists
                    if rcs[0] == si.TCS_OK:
                        ok.add(code)
                want = set(si.TABLE.get(kind, ()))
                assert ok == want, (kind, "library only:", sorted(ok - want), "table only:", sorted(want - ok))
                seen_kinds += bool(want)
    assert seen_kinds == sum(1 for k in si.KINDS if k[2] == epilogue)


def test_table_is_well_formed():
    space = set(si.code_space())
    for kind, codes in si.TABLE.items():
        assert len(set(codes)) == len(codes) and set(codes) <= space, kind
    assert len(si.all_instances()) == sum(len(v) for v in si.TABLE.values())
    assert len(si.table_keys()) == 2 * len(si.all_instances())


def test_heuristic_picks_table_instances_for_the_loop_layers():
    """tile_cfg = 0 at the BASELINE shapes (640x480 and the KITTI shape; batch 1, 4, 8): the library's own choice for each of the
    loop's layers is an instance of the table, for both product counts."""
    native, lib = _lib()
    picks = {}
    for (name, ksize, stride, epi, taps, cins, cout, div) in si.LOOP_LAYERS:
        for image in si.IMAGES:
            H, W = si.layer_grid(image, div)
            for B in si.BATCHES:
                for products in (0, 1):
                    d = si.host_desc(native, ksize, stride, epi, taps, cins, cout, H, W, B=B, products=products)
                    rc, p = si.plan(native, lib, d)
                    assert rc == si.TCS_OK, (name, image, B, rc)
                    assert si.instance_key(p) in si.table_keys(), (name, image, B, si.instance_key(p))
                    assert (p.ksize, p.stride, p.epilogue, p.taps) == (ksize, stride, epi, taps)
                    picks[(name, image, B)] = (p.row_split, p.rows_per_wave, p.mt, p.rows, p.ksteps, p.nstage)
    # the choice depends on the grid and on the batch (the block count): more than one instance is reached per epilogue kind
    assert len({v for (n, _, _), v in picks.items() if n == "gru08.q"} | {v for (n, _, _), v in picks.items() if n == "gru32.q"}) >= 2
