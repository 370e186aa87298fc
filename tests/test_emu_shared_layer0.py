"""Round 8 on the CPU emulator: the paired layer-0 in_proj of a guided trans_enc forward (csrc/gemm_x3.h PAIR; include/mdm_hip.h
MDM_OPT_ENC_SHARED_LAYER0) against the one-tile-per-sequence launch -- bit for bit, in the emulator's EARLY mode (this process) and
in its LATE mode (a child interpreter: the mode is latched per process, tests/test_emu_late.py), and with every engine buffer
pre-filled with NaN (tests/test_emu_poison.py's idiom): a plane row the paired epilogue never writes, or a statistic read from a row it
should not have touched, shows as NaN or as a difference.  Shapes: S + 1 < 208 with two tiles per workgroup (B = 2 samples x 3 column
tiles on the emulator's 3 persistent workgroups), S = 32 (tile row S opens a sub-tile past the planes' key tiles) and S = 207 (the
shared row is the tile's last row)."""
import os
import subprocess
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
from emu_lib import emu  # noqa: E402
from helpers import make_pair, maxabs, orc, small_state_dict, synth_y  # noqa: E402

SHAPES = [(2, 33, [33, 5]), (1, 31, [17]), (1, 206, [150])]


def _guided(lib, engine_options, shared, B, T, lengths, layers=1):
    engine_options(small_gemm_max_seqs=0, enc_shared_layer0=shared)
    sd = small_state_dict(num_layers=layers)
    model, _ = make_pair(sd, 2, "cpu", guided=True, native_lib=lib, precision="f16x3")
    y = synth_y(B, T, seed=2, lengths=lengths)
    x = torch.randn(B, 263, 1, T, generator=torch.Generator().manual_seed(0))
    t = torch.tensor([1, 0][:B])
    out = model(x, t, y=dict(y))
    assert model.model.engine().get_option("enc_shared_layer0") == shared
    return out, (sd, x, t, y)


@pytest.mark.parametrize("B,T,lengths", SHAPES)
def test_emulated_shared_layer0_in_proj_is_bit_identical(engine_options, B, T, lengths):
    lib = emu()
    on, (sd, x, t, y) = _guided(lib, engine_options, 1, B, T, lengths)
    off, _ = _guided(lib, engine_options, 0, B, T, lengths)
    assert torch.equal(on, off), maxabs(on, off)
    assert maxabs(on, orc.cfg_forward(sd, x, t, y, num_heads=2)) < 2e-5


@pytest.fixture()
def poisoned(monkeypatch):
    import mdm_amd._engine as eng_mod
    real = torch

    class PoisonTorch(types.ModuleType):
        def __getattr__(self, k):
            return getattr(real, k)

        def empty(self, *a, **k):
            t = real.empty(*a, **k)
            return t.fill_(0xFF) if t.dtype == real.uint8 else (t.fill_(float("nan")) if t.is_floating_point() else t)

        def empty_like(self, x, **k):
            t = real.empty_like(x, **k)
            return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(eng_mod, "torch", PoisonTorch("torch"))
    return emu()


@pytest.mark.parametrize("B,T,lengths", [SHAPES[0], SHAPES[2]])
def test_emulated_shared_layer0_in_proj_reads_nothing_it_did_not_write(poisoned, engine_options, B, T, lengths):
    """Two layers: the second one's folded in_proj / residual GEMMs read what layer 0 left behind."""
    on, (sd, x, t, y) = _guided(poisoned, engine_options, 1, B, T, lengths, layers=2)
    assert not bool(torch.isnan(on).any())
    off, _ = _guided(poisoned, engine_options, 0, B, T, lengths, layers=2)
    assert torch.equal(on, off), maxabs(on, off)
    assert maxabs(on, orc.cfg_forward(sd, x, t, y, num_heads=2)) < 2e-5


@pytest.mark.slow
def test_emulated_shared_layer0_in_proj_under_the_late_async_model():
    """The bit-identity cases again with MDM_EMU_LATE=1: every asynchronous operation is withheld until the counted wait that covers
    it, so a paired tile whose changed source offset needed another wait count would read a stale row."""
    emu()                                              # build once, in this process
    env = dict(os.environ, MDM_EMU_LATE="1", MDM_TEST_SERIAL="1", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    env.pop("PYTEST_XDIST_WORKER", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "test_emulated_shared_layer0_in_proj_is_bit_identical"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=3000)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, tail
    assert "3 passed" in tail and "failed" not in tail, tail
