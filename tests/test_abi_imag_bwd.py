"""sd_imagine_bwd's descriptor (sd_imagine_bwd_desc: C gives a typedef and a function one namespace, so the struct
cannot carry the entry's name) has the ctypes layout of the C struct (gcc-compiled sizeof / offsetof probes, as
tests/test_abi.py does for sd_imagine), and its shape gate answers on a host-only descriptor."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sdhip.h")
PROBE = ["N", "img_layers", "eps", "seed", "seed_ptr", "row_offset", "Wa", "Wao", "Wi", "Wl", "feats", "gates",
         "img_pre", "act_rstd", "plogit", "d_stoch", "d_deter", "work", "t_begin", "t_end"]


def test_desc_layout_matches_c():
    from sdreamer import _native as nat
    S, cname = nat.ImagineBwdDesc, "sd_imagine_bwd_desc"
    assert S._fields_[0][0] == PROBE[0] and S._fields_[-1][0] == PROBE[-1]  # the first and the last field are probed
    fmt = " ".join(["%zu"] * (len(PROBE) + 1))
    args = ", ".join([f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in PROBE])
    src = f'#include <stdio.h>\n#include <stddef.h>\n#include "sdhip.h"\nint main(void){{printf("{fmt}", {args}); return 0;}}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in PROBE]


def _desc(D, G, S, K, A=6, discrete=False, actor_layers=3, img_layers=2, N=64, H1=3):
    from sdreamer import _native as nat
    d = nat.ImagineBwdDesc()
    d.N, d.H1, d.D, d.U, d.SK, d.Kd, d.G, d.A = N, H1, D, 256, S * K, K, G, A
    d.act_discrete, d.actor_layers, d.img_layers = int(discrete), actor_layers, img_layers
    return d


def test_gate_on_host_only_descriptors():
    """no pointer is set: the gate reads shapes only, launches nothing and touches no device"""
    from sdreamer import _native as nat
    ok, floats, run = (nat.fns[n] for n in ("sd_imagine_bwd_ok", "sd_imagine_bwd_work_floats", "sd_imagine_bwd"))
    good = _desc(2048, 8, 32, 16)
    assert ok(ctypes.addressof(good)) == 1 and floats(ctypes.addressof(good)) > 0
    assert run(ctypes.addressof(good), 0) == -1  # SD_EARG: admitted shape, null pointers; refused before any launch
    for bad in (_desc(768, 8, 4, 16), _desc(256, 8, 4, 16), _desc(2048, 8, 32, 16, H1=1), _desc(2048, 8, 32, 64)):
        assert ok(ctypes.addressof(bad)) == 0
        assert floats(ctypes.addressof(bad)) == nat.SD_ESHAPE
        assert run(ctypes.addressof(bad), 0) == nat.SD_ESHAPE
    assert ok(0) == 0
    # the gate is sd_imagine's own (plus H1 >= 2): the same answers over the small cases' shapes
    import small_models as sm
    for c in sm.IMAG_CASES:
        d = _desc(c.D, c.G, c.S, c.K, c.A, c.discrete, c.actor_layers, c.img_layers, c.N, c.H1)
        fwd = sm.imagine_work_status(c.D, c.G, c.S, c.K, c.A, c.discrete, c.actor_layers, c.img_layers, c.N, c.H1)
        assert (ok(ctypes.addressof(d)) == 1) == (fwd > 0) == c.fused, c.name
