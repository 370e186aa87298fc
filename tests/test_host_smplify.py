"""mdm_amd/simplify_loc2rot.py without a GPU: the loader's errors, the preparation of the mixture prior against MaxMixturePrior's own
buffers, the float64 oracle of tests/smplify_helpers.py pinned to the reference's own functions (tests/golden/smplify_value_grad.npz),
and the C++ restatement of torch's strong-Wolfe line search against recorded searches of torch's own."""
import ctypes as C
import pickle

import numpy as np
import pytest

import smplify_helpers as H
import smpl_mesh_helpers as smh


def _files(tmp_path, gmm=None):
    fields, extra, _ids, _maps = smh.fixture_model()
    model_path, _ = smh.write_model_files(tmp_path, fields, extra)
    return model_path, H.write_gmm(tmp_path / "prior", gmm)


def _emu():
    from emu.emu_lib import emu
    return emu()


def test_loader_errors(tmp_path, monkeypatch):
    from mdm_amd import simplify_loc2rot as s2r
    model_path, gmm_path = _files(tmp_path)
    kw = dict(cuda=False, smpl_model_path=model_path, mean_params=H.mean_params(), _native_lib=_emu())
    with pytest.raises(FileNotFoundError, match="gmm_08.pkl"):
        s2r.joints2smpl(3, 0, gmm_path=str(tmp_path / "nowhere" / "gmm_08.pkl"), **kw)
    # no h5py and no mean_params: the message names the file and the argument
    import builtins
    real_import = builtins.__import__

    def no_h5py(name, *a, **k):
        if name == "h5py":
            raise ImportError("No module named 'h5py'")
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_h5py)
    with pytest.raises(ImportError, match=r"neutral_smpl_mean_params\.h5.*mean_params="):
        s2r.joints2smpl(3, 0, gmm_path=gmm_path, **dict(kw, mean_params=None))
    monkeypatch.setattr(builtins, "__import__", real_import)
    with pytest.raises(ValueError, match=r"pose\[72\]"):
        s2r.joints2smpl(3, 0, gmm_path=gmm_path, **dict(kw, mean_params=(np.zeros(69), np.zeros(10))))
    # 21 joints instead of 22
    fit = s2r.joints2smpl(3, 0, gmm_path=gmm_path, **kw)
    with pytest.raises(ValueError, match=r"\[num_frames, 22, 3\]"):
        fit.joint2smpl(np.zeros((3, 21, 3), np.float32))
    # a mixture of the wrong width
    g = H.synthetic_gmm()
    bad = dict(means=g["means"][:, :63], covars=g["covars"][:, :63, :63], weights=g["weights"])
    narrow = H.write_gmm(tmp_path / "narrow", bad)
    with pytest.raises(ValueError, match=r"means \[8, 69\]"):
        s2r.joints2smpl(3, 0, gmm_path=narrow, **kw).joint2smpl(np.zeros((3, 22, 3), np.float32))
    with open(str(tmp_path / "list.pkl"), "wb") as f:
        pickle.dump([1, 2], f)
    with pytest.raises(ValueError, match="expected a dict"):
        s2r.load_gmm(str(tmp_path / "list.pkl"))


def test_the_product_library_refuses_a_host_device(tmp_path):
    """No CPU fallback: with the product library a host device is refused like everywhere else (the library itself need not load)."""
    from mdm_amd import _native as nat
    from mdm_amd import simplify_loc2rot as s2r
    model_path, gmm_path = _files(tmp_path)

    class Product:
        path = nat.LIB_PATH
    fit = s2r.joints2smpl(3, 0, cuda=False, smpl_model_path=model_path, gmm_path=gmm_path, mean_params=H.mean_params(), _native_lib=Product())
    with pytest.raises(nat.MdmError, match="needs the joints on a cuda"):
        fit.joint2smpl(np.zeros((3, 22, 3), np.float32))


def test_prior_preparation_equals_the_references_buffers_bit_for_bit():
    from mdm_amd import simplify_loc2rot as s2r
    got, want = s2r.prepare_gmm(H.synthetic_gmm()), H.fixture("prior")
    for k in ("means", "precisions", "nll_weights"):
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    # -log(nll_weights) in torch's float32 log, as merged_log_likelihood takes it
    assert np.abs(got["neg_log_nll_weights"] + np.log(want["nll_weights"].astype(np.float64)).reshape(8)).max() < 1e-5
    assert np.isfinite(got["neg_log_nll_weights"]).all()


def test_the_synthetic_inputs_are_the_fixtures_and_meet_their_conditions():
    fx, inp = H.fixture("value_grad"), H.value_grad_inputs()
    for k, v in inp.items():
        assert np.array_equal(fx[k], v), k
    winners, margin = H.check_input_conditions(fx, H.prior64())
    print(f"[smplify host] winning mixture components {winners}, smallest relative margin {margin:.3e}")
    for T in (3, H.F + 1):
        assert np.array_equal(H.fixture("fit_short_T%d" % T)["j3d"], H.fit_targets(T, 100 + T))


@pytest.mark.parametrize("stage,kind", [(1, "ones"), (2, "ones"), (2, "foot")])
def test_the_oracle_is_pinned_to_the_references_own_functions(stage, kind):
    """The reference's float32 per-frame losses, total and autograd gradient against the float64 oracle: the error IS e_ref of the
    pin report, and it is what float32 gives on sums of this size (well below 1e-4)."""
    fx = H.fixture("value_grad")
    frames64, g64 = H.shared_oracle(stage, kind)
    pre = "s1_" if stage == 1 else "s2_%s_" % kind
    ev, eg = H.errors_against_oracle(stage, fx[pre + "frames"], H.per_frame_grad(stage, fx[pre + "grad"], H.NF), frames64, g64)
    et = abs(float(fx[pre + "total"]) - frames64.sum()) / frames64.sum()
    ref = H.pin_report()["value_grad"]["stage%d_%s" % (stage, kind)]
    print(f"[smplify host] stage {stage} conf={kind}: the reference's float32 against the oracle: value {ev:.3e} gradient {eg:.3e} total {et:.3e}")
    assert ev == pytest.approx(ref["value"], rel=1e-6) and eg == pytest.approx(ref["grad"], rel=1e-6)
    assert ev < 1e-4 and eg < 1e-4 and et < 1e-4
    if stage == 1:      # guess_init_3d: the mean offset of joints (2, 1, 17, 16), restated on the oracle's joints
        import torch
        with torch.no_grad():
            mj = H.model_joints(torch.tensor(np.concatenate([fx["go"], fx["body"]], 1).astype(np.float64)),
                                torch.tensor(fx["betas"].astype(np.float64)), H.tables64(H.model_fields())).numpy()
        sel = [2, 1, 17, 16]
        guess = (fx["j3d"][:, sel].astype(np.float64) - mj[:, sel]).sum(1) / 4.0
        assert np.abs(guess - fx["s1_guess"]).max() < 1e-5


def test_the_line_search_follows_torchs_strong_wolfe_step_for_step():
    """mdm_smplify_strong_wolfe replays recorded searches of torch.optim.lbfgs._strong_wolfe: the same steps, exactly, the same number
    of evaluations and the same result -- with float64 tensors (double on both sides) and, the cases ending in _f32, with g . d and
    max|d| as 0-dim float32 tensors, the mixed arithmetic a fit runs on."""
    lib = _emu()
    fx = H.fixture("linesearch")
    for name, seq, head in zip(fx["names"], fx["seq"], fx["head"]):
        t0, f0, gtd0, max_ls, n, t_fin, f_fin, f32 = head
        n = int(n)
        f_seq = (C.c_double * n)(*seq[1, :n])
        g_seq = (C.c_double * n)(*seq[2, :n])
        t_seq = (C.c_double * n)()
        n_evals, t_out, f_out = C.c_int32(), C.c_double(), C.c_double()
        rc = lib.mdm_smplify_strong_wolfe(f_seq, g_seq, n, t0, f0, gtd0, 1.0, 1e-9, int(max_ls), int(f32), t_seq, C.byref(n_evals), C.byref(t_out),
                                          C.byref(f_out))
        assert rc == 0, lib.mdm_last_error()
        print(f"[smplify host] line search {name}: {n_evals.value} evaluations (recorded {n}), steps {list(t_seq)}")
        assert n_evals.value == n and list(t_seq) == list(seq[0, :n]), name
        assert t_out.value == t_fin and f_out.value == f_fin, name
    # a sequence that is too short is an error, not a read past its end
    rc = lib.mdm_smplify_strong_wolfe((C.c_double * 1)(5.0), (C.c_double * 1)(1.0), 1, 1.0, 0.0, -1.0, 1.0, 1e-9, 25, 0, (C.c_double * 1)(),
                                      C.byref(C.c_int32()), C.byref(C.c_double()), C.byref(C.c_double()))
    assert rc == -1 and b"more evaluations" in lib.mdm_last_error()
