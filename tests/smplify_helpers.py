"""Shared scaffolding of the SMPLify tests (mdm_amd/simplify_loc2rot.py, csrc/smplify.h): the reference-pinned fixtures
(tests/golden/smplify_*.npz, tools/make_golden_smplify.py), a float64 torch restatement of the two fitting losses with autograd -- the
oracle --, the synthetic mixture prior and inputs, and the checks the emulator and the GPU tests share.

Yardsticks (tests/golden/PIN_REPORT_smplify.json carries them; the tool measured them on the reference's own code):
  value and gradient   e_ref = the error of the reference's float32 value (relative, per frame) and gradient (max-abs over max|g|)
                       against the float64 oracle on the same inputs, pooled over the 65 frames of a case; bound 4 x e_ref.
  short horizon        e_ref = the largest deviation, per output, of eight runs of the reference on targets scaled by 1 + k 2^-23
                       (k = +-1 .. +-4) from its unperturbed run; bound 4 x e_ref.
  whole fit            final loss <= reference x (1 + 4 x the ensemble's relative spread); worst joint-to-target distance <= the
                       ensemble's worst + 4 x its spread.  A better fit is never a failure."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import torch

import smpl_mesh_helpers as smh
from smpl_helpers import GOLDEN, SMPL_PARENTS

F = 32                                        # csrc/smplify.h SMF_FRAMES
FRAME_COUNTS = (1, F - 1, F, F + 1, 2 * F + 1)
NF = 2 * F + 1
CASES = [(1, "ones"), (F - 1, "ones"), (F, "ones"), (F + 1, "foot"), (2 * F + 1, "ones"), (2 * F + 1, "foot")]
FACTOR = 4.0
MEAN_SEED, GMM_SEED = 5, 11
WEIGHTS = dict(joint=600.0, sigma=100.0, prior=4.78 * 1.5, angle=15.2, shape=5.0, preserve=5.0, depth=100.0)
# the frames of the value / gradient inputs that carry an operand regime
REGIMES = dict(zero_pose=1, near_pi=2, angle_3=3, past_knee=4, betas_pm3=5)


def fixture(name):
    return np.load(os.path.join(GOLDEN, "smplify_" + name + ".npz"))


def pin_report():
    with open(os.path.join(GOLDEN, "PIN_REPORT_smplify.json")) as f:
        return json.load(f)


def conf_of(kind):
    c = np.ones(22, np.float32)
    if kind == "foot":
        c[[7, 8, 10, 11]] = 1.5
    return c


# ---- the synthetic model ---------------------------------------------------------------------------------------------------------
def model_fields():
    """The 48-vertex synthetic SMPL model every SMPL fixture of this project was made on (tests/golden/smpl_mesh_model.npz)."""
    return smh.fixture_model()[0]


def tables64(fields):
    reg = np.asarray(fields["J_regressor"], np.float64)
    return dict(j0=reg @ np.asarray(fields["v_template"], np.float64),
                jdirs=np.einsum("jv,vcl->jcl", reg, np.asarray(fields["shapedirs"], np.float64)[:, :, :10]),
                parents=list(SMPL_PARENTS))


def synthetic_gmm(seed=GMM_SEED):
    """A random 8 x 69 mixture: means ~ N(0, 0.3), covariances Q diag(lambda) Q^T with lambda log-uniform in [0.01, 0.5]."""
    g = np.random.default_rng(seed)
    means = g.normal(0, 0.3, (8, 69))
    covs = []
    for _ in range(8):
        q, _r = np.linalg.qr(g.normal(size=(69, 69)))
        lam = np.exp(g.uniform(np.log(0.01), np.log(0.5), 69))
        c = (q * lam) @ q.T
        covs.append(0.5 * (c + c.T))
    w = g.random(8) + 0.5
    return dict(means=means, covars=np.stack(covs), weights=w / w.sum())


def write_gmm(folder, gmm=None):
    os.makedirs(str(folder), exist_ok=True)
    path = os.path.join(str(folder), "gmm_08.pkl")
    with open(path, "wb") as f:
        pickle.dump(synthetic_gmm() if gmm is None else gmm, f, protocol=2)
    return path


def mean_params(seed=MEAN_SEED):
    g = np.random.default_rng(seed)
    return g.normal(0, 0.15, 72).astype(np.float32), g.normal(0, 0.3, 10).astype(np.float32)


def prior64():
    """The prior the reference evaluates: MaxMixturePrior's float32 buffers (the fixture's), promoted."""
    p = fixture("prior")
    return dict(means=p["means"].astype(np.float64), prec=p["precisions"].astype(np.float64),
                nlw=-np.log(p["nll_weights"].astype(np.float64).reshape(8)))


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------------
def batch_rodrigues(rv):
    """smplx 0.1.28 lbs.batch_rodrigues, any dtype: [N, 3] -> [N, 3, 3]."""
    angle = torch.norm(rv + 1e-8, dim=1, keepdim=True)
    rot_dir = rv / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = torch.split(rot_dir, 1, dim=1)
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    return torch.eye(3, dtype=rv.dtype, device=rv.device)[None] + sin * K + (1 - cos) * torch.bmm(K, K)


def model_joints(pose, betas, tab):
    """The 24 posed joints of smplx's SMPL forward: pose [T, 72] axis-angle, betas [T, 10] -> [T, 24, 3]."""
    T = pose.shape[0]
    dt = pose.dtype
    J = torch.as_tensor(tab["j0"], dtype=dt)[None] + torch.einsum("jcl,tl->tjc", torch.as_tensor(tab["jdirs"], dtype=dt), betas)
    R = batch_rodrigues(pose.reshape(-1, 3)).view(T, 24, 3, 3)
    par = tab["parents"]
    GR, Gt = [R[:, 0]], [J[:, 0]]
    for i in range(1, 24):
        GR.append(GR[par[i]] @ R[:, i])
        Gt.append(torch.einsum("trk,tk->tr", GR[par[i]], J[:, i] - J[:, par[i]]) + Gt[par[i]])
    return torch.stack(Gt, dim=1)


def prior_ll(body, pr):
    """merged_log_likelihood's [T, 8] table before the min."""
    d = body[:, None, :] - torch.as_tensor(pr["means"], dtype=body.dtype)
    pd = torch.einsum("mij,bmj->bmi", torch.as_tensor(pr["prec"], dtype=body.dtype), d)
    return 0.5 * (pd * d).sum(-1) + torch.as_tensor(pr["nlw"], dtype=body.dtype)


def stage1_frames(go, cam, body, betas, cam_est, j3d, tab, w=WEIGHTS):
    """camera_fitting_loss_3d per frame [T] (the depth term four times, as the reference's broadcast counts it)."""
    mj = model_joints(torch.cat([go, body], 1), betas, tab) + cam[:, None]
    sel = [2, 1, 17, 16]
    err = (j3d[:, sel] - mj[:, sel]) ** 2
    depth = (w["depth"] ** 2) * (cam - cam_est) ** 2
    return (err + depth[:, None]).sum((1, 2))


def stage2_frames(body, betas, go, cam, preserve, j3d, conf, tab, pr, w=WEIGHTS):
    """body_fitting_loss_3d per frame [T] as smplify.py:226-233 calls it."""
    mj = model_joints(torch.cat([go, body], 1), betas, tab)[:, :22] + cam[:, None]
    x2 = (mj - j3d) ** 2
    s2 = w["sigma"] ** 2
    joint = ((w["joint"] ** 2) * ((conf ** 2) * ((s2 * x2) / (s2 + x2)).sum(-1))).sum(-1)
    prior = (w["prior"] ** 2) * prior_ll(body, pr).min(1)[0]
    sign = torch.tensor([1., -1., -1., -1.], dtype=body.dtype, device=body.device)
    angle = (w["angle"] ** 2) * (torch.exp(body[:, [52, 55, 9, 12]] * sign) ** 2).sum(-1)
    shape = (w["shape"] ** 2) * (betas ** 2).sum(-1)
    keep = (w["preserve"] ** 2) * ((body - preserve) ** 2).sum(-1)
    return joint + prior + angle + shape + keep


def oracle(stage, inp, conf, T, tab, pr):
    """(per-frame loss [T], flat gradient [n], total) in float64 at the first T frames of the inputs `inp` (a fixture or a dict)."""
    t64 = lambda k, grad=False: torch.tensor(np.asarray(inp[k][:T], np.float64), requires_grad=grad)       # noqa: E731
    go, cam = t64("go", True), t64("cam", True)
    if stage == 1:
        frames = stage1_frames(go, cam, t64("body"), t64("betas"), t64("cam_est"), t64("j3d"), tab)
        frames.sum().backward()
        grad = torch.cat([go.grad.reshape(-1), cam.grad.reshape(-1)])
    else:
        body, betas = t64("body", True), t64("betas", True)
        frames = stage2_frames(body, betas, go, cam, t64("preserve"), t64("j3d"), torch.tensor(conf, dtype=torch.float64), tab, pr)
        frames.sum().backward()
        grad = torch.cat([body.grad.reshape(-1), betas.grad.reshape(-1), go.grad.reshape(-1), cam.grad.reshape(-1)])
    return frames.detach().numpy(), grad.numpy(), float(frames.detach().sum())


def flat(stage, inp, T, what=None):
    parts = ("go", "cam") if stage == 1 else ("body", "betas", "go", "cam")
    return np.concatenate([np.asarray(inp[(what + "_" if what else "") + k][:T], np.float32).reshape(-1) for k in parts])


def per_frame_grad(stage, g, T):
    """[T, 6 or 85]: the entries of the flat gradient that belong to each frame."""
    widths = (3, 3) if stage == 1 else (69, 10, 3, 3)
    out, at = [], 0
    for wd in widths:
        out.append(np.asarray(g[at:at + T * wd]).reshape(T, wd))
        at += T * wd
    return np.concatenate(out, 1)


def value_grad_inputs(seed=23):
    """The 65 frames of the value / gradient cases (float32-exact).  Body poses sit near the mixture's means, a different component
    from frame to frame; the targets are the model's joints at a nearby pose plus a translation and 5 mm of noise; REGIMES names the
    frames that carry an operand regime."""
    g = np.random.default_rng(seed)
    gm = synthetic_gmm()
    tab = tables64(model_fields())
    comp = (np.arange(NF) * 3) % 8
    body = gm["means"][comp] + g.normal(0, 0.05, (NF, 69))
    go, betas = g.normal(0, 0.3, (NF, 3)), g.normal(0, 0.5, (NF, 10))
    body[REGIMES["zero_pose"]] = 0.0
    go[REGIMES["zero_pose"]] = 0.0
    ax = np.array([0.6, -0.48, 0.64])
    body[REGIMES["near_pi"], 15:18] = ax * (np.pi - 1e-3)          # joint 6
    body[REGIMES["angle_3"], 24:27] = ax[::-1] * 3.0               # joint 9
    betas[REGIMES["betas_pm3"]] = np.where(np.arange(10) % 2 == 0, 3.0, -3.0)
    trans = g.normal(0, 0.3, (NF, 3))
    with torch.no_grad():
        tj = model_joints(torch.tensor(np.concatenate([go, body], 1) + g.normal(0, 0.1, (NF, 72))),
                          torch.tensor(betas + g.normal(0, 0.2, (NF, 10))), tab).numpy()
    j3d = tj[:, :22] + trans[:, None] + g.normal(0, 0.005, (NF, 22, 3))
    j3d[REGIMES["past_knee"], 5, 0] += 150.0
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)       # noqa: E731
    return dict(body=f32(body), betas=f32(betas), go=f32(go), cam=f32(trans + g.normal(0, 0.05, (NF, 3))),
                preserve=f32(body + g.normal(0, 0.1, (NF, 69))), cam_est=f32(trans + g.normal(0, 0.02, (NF, 3))), j3d=f32(j3d),
                dir_body=f32(g.normal(0, 1, (NF, 69))), dir_betas=f32(g.normal(0, 1, (NF, 10))), dir_go=f32(g.normal(0, 1, (NF, 3))),
                dir_cam=f32(g.normal(0, 1, (NF, 3))))


def check_input_conditions(inp, pr):
    """Conditions on the INPUTS, checked on the CPU in float64: at least three mixture components win somewhere, and every frame's
    two best components differ by more than 1e-3 relative."""
    ll = prior_ll(torch.tensor(inp["body"].astype(np.float64)), pr).numpy()
    order = np.sort(ll, 1)
    margin = (order[:, 1] - order[:, 0]) / np.abs(order[:, 0])
    winners = sorted(set(ll.argmin(1).tolist()))
    assert len(winners) >= 3 and margin.min() > 1e-3, (winners, margin.min())
    return winners, float(margin.min())


def fit_targets(T, seed):
    """Targets of a fit: the model's joints at random poses (sigma = 0.3 rad) and betas (sigma = 0.5), plus a translation and 5 mm of noise."""
    g = np.random.default_rng(seed)
    tab = tables64(model_fields())
    with torch.no_grad():
        tj = model_joints(torch.tensor(g.normal(0, 0.3, (T, 72))), torch.tensor(g.normal(0, 0.5, (T, 10))), tab).numpy()
    return np.ascontiguousarray(tj[:, :22] + g.normal(0, 0.5, (1, 1, 3)) + g.normal(0, 0.005, (T, 22, 3)), dtype=np.float32)


# ---- the library under test ------------------------------------------------------------------------------------------------------
class Bench:
    """The prepared model on `dev` ('cpu': the emulator's host pointers) and the raw C-ABI calls."""

    def __init__(self, lib, dev):
        from mdm_amd import _native as nat
        from mdm_amd import simplify_loc2rot as s2r
        self.nat, self.lib, self.dev = nat, lib, torch.device(dev)
        tab = tables64(model_fields())
        g = s2r.prepare_gmm(synthetic_gmm())
        host = dict(j0=tab["j0"].astype(np.float32), jdirs=tab["jdirs"].astype(np.float32), means=g["means"], precisions=g["precisions"],
                    neg_log_nll_weights=g["neg_log_nll_weights"])
        self.tabs = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.dev) for k, v in host.items()}
        self.parents = np.array([-1] + SMPL_PARENTS[1:], np.int32)
        self.model = nat.MdmSmplifyModel(parents=self.parents.ctypes.data_as(C.POINTER(C.c_int32)),
                                         **{k: v.data_ptr() for k, v in self.tabs.items()})

    def stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else None

    def to(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    def workspace(self, call, T, poison=None):
        n = self.lib.mdm_smplify_workspace_bytes(C.byref(self.model), C.byref(call), T)
        assert n > 0, self.lib.mdm_last_error()
        ws = torch.empty(n, dtype=torch.uint8, device=self.dev)
        if poison is not None:
            ws.fill_(poison)
        return ws, n

    def value_grad(self, stage, inp, conf, T, frames=None, poison=None, fill=0.0, stream=None, expect_rc=0):
        """mdm_smplify_value_grad at frames [0, T) of `inp` (or at the listed frames).  Returns numpy outputs."""
        sel = np.arange(T) if frames is None else np.asarray(frames)
        T = len(sel)
        keys = ("body", "betas", "go", "cam", "preserve", "cam_est", "j3d", "dir_body", "dir_betas", "dir_go", "dir_cam")
        sub = {k: np.asarray(inp[k])[sel] for k in keys}
        call = self.nat.MdmSmplifyCall()
        x, d = self.to(flat(stage, sub, T)), self.to(flat(stage, sub, T, "dir"))
        fixed = self.to(sub["body"] if stage == 1 else sub["preserve"])
        betas, cam_est, j3d, cf = self.to(sub["betas"]), self.to(sub["cam_est"]), self.to(sub["j3d"]), self.to(conf)
        n = T * (6 if stage == 1 else 85)
        grad = torch.full((n,), fill, dtype=torch.float32, device=self.dev)
        terms = torch.full((T, 6), fill, dtype=torch.float32, device=self.dev)
        joints = torch.full((T, 24, 3), fill, dtype=torch.float32, device=self.dev)
        scal = (C.c_float * 3)(*([fill] * 3))
        ws, nbytes = self.workspace(call, T, poison)
        rc = self.lib.mdm_smplify_value_grad(C.byref(self.model), C.byref(call), stage, x.data_ptr(), d.data_ptr(), fixed.data_ptr(),
                                             betas.data_ptr(), cam_est.data_ptr(), j3d.data_ptr(), cf.data_ptr(), T, grad.data_ptr(),
                                             terms.data_ptr(), joints.data_ptr(), scal, ws.data_ptr(), nbytes,
                                             self.stream() if stream is None else stream)
        assert rc == expect_rc, (rc, self.lib.mdm_last_error())
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return dict(grad=grad.cpu().numpy(), terms=terms.cpu().numpy(), joints=joints.cpu().numpy(), scalars=np.array(list(scal), np.float32),
                    dir=d.cpu().numpy())

    def fit(self, j3d, conf, call, init=None, poison=None):
        T = j3d.shape[0]
        pose0, shape0 = mean_params()
        if init is None:
            init = (np.tile(pose0, (T, 1)), np.tile(shape0, (T, 1)))
        ip, ib, jd, cf = self.to(init[0]), self.to(init[1]), self.to(j3d), self.to(conf)
        out = dict(pose=(T, 72), betas=(T, 10), cam=(T, 3), joints=(T, 24, 3), thetas=(1, 25, 6, T))
        o = {k: torch.full(s, float("nan"), dtype=torch.float32, device=self.dev) for k, s in out.items()}
        stats = (C.c_double * 6)()
        ws, nbytes = self.workspace(call, T, poison)
        rc = self.lib.mdm_smplify_fit(C.byref(self.model), C.byref(call), ip.data_ptr(), ib.data_ptr(), jd.data_ptr(), cf.data_ptr(), T,
                                      o["pose"].data_ptr(), o["betas"].data_ptr(), o["cam"].data_ptr(), o["joints"].data_ptr(),
                                      o["thetas"].data_ptr(), stats, ws.data_ptr(), nbytes, self.stream())
        assert rc == 0, (rc, self.lib.mdm_last_error())
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in o.items()}
        res["stats"] = np.array(list(stats))
        return res


_ORACLE = {}


def shared_oracle(stage, kind):
    """The float64 oracle at all 65 frames, computed once per (stage, confidence) and shared by the tests."""
    if (stage, kind) not in _ORACLE:
        inp = fixture("value_grad")
        pr = prior64()
        check_input_conditions(inp, pr)
        frames, grad, _ = oracle(stage, inp, conf_of(kind), NF, tables64(model_fields()), pr)
        _ORACLE[(stage, kind)] = (frames, per_frame_grad(stage, grad, NF))
    return _ORACLE[(stage, kind)]


def errors_against_oracle(stage, frames32, gframes32, frames64, gframes64):
    """(value: the largest per-frame relative error, gradient: max-abs over max|g|)."""
    ev = float(np.max(np.abs(frames32.astype(np.float64) - frames64) / np.abs(frames64)))
    eg = float(np.abs(gframes32.astype(np.float64) - gframes64).max() / np.abs(gframes64).max())
    return ev, eg


def check_value_grad(bench, stage, T, kind, tag):
    """One case: the first T frames against the oracle, within 4 x e_ref of the reference's own float32 error."""
    inp = fixture("value_grad")
    frames64, g64 = shared_oracle(stage, kind)
    got = bench.value_grad(stage, inp, conf_of(kind), T)
    gf = per_frame_grad(stage, got["grad"], T)
    ev, eg = errors_against_oracle(stage, got["terms"][:, 5], gf, frames64[:T], g64[:T])
    ref = pin_report()["value_grad"]["stage%d_%s" % (stage, kind)]
    total64 = float(frames64[:T].sum())
    et = abs(float(got["scalars"][0]) - total64) / abs(total64)
    gmax64 = float(np.abs(g64[:T]).max())
    em = abs(float(got["scalars"][1]) - gmax64) / gmax64
    gd64 = float((g64[:T] * per_frame_grad(stage, got["dir"], T).astype(np.float64)).sum())
    scale = float(np.abs(g64[:T] * per_frame_grad(stage, got["dir"], T)).sum())
    ed = abs(float(got["scalars"][2]) - gd64) / scale
    print(f"[smplify {tag}] stage {stage} T={T} conf={kind}: value {ev:.3e} (e_ref {ref['value']:.3e}, ratio {ev / ref['value']:.2f}) "
          f"gradient {eg:.3e} (e_ref {ref['grad']:.3e}, ratio {eg / ref['grad']:.2f}) total {et:.3e} max|g| {em:.3e} g.d {ed:.3e}")
    assert np.isfinite(got["grad"]).all() and np.isfinite(got["terms"]).all()
    assert ev <= FACTOR * ref["value"] and et <= FACTOR * ref["value"], (ev, et, ref)
    assert eg <= FACTOR * ref["grad"] and em <= FACTOR * ref["grad"] and ed <= FACTOR * ref["grad"], (eg, em, ed, ref)
    # the model joints the kernel reports are those of the oracle's chain
    with torch.no_grad():
        mj = model_joints(torch.tensor(np.concatenate([inp["go"][:T], inp["body"][:T]], 1).astype(np.float64)),
                          torch.tensor(inp["betas"][:T].astype(np.float64)), tables64(model_fields())).numpy()
    ej = float(np.abs(got["joints"] - mj).max())
    print(f"[smplify {tag}] model joints max-abs {ej:.3e}")
    assert ej <= 1e-5, ej


def check_position_invariance(bench, stage, tag):
    """Every one of the 65 frames alone (T = 1) and at its place in the 65-frame batch -- every lane and workgroup slot --: the same bits
    of its terms and gradient; and the batch in reverse order."""
    inp = fixture("value_grad")
    conf = conf_of("ones")
    full = bench.value_grad(stage, inp, conf, NF)
    gf = per_frame_grad(stage, full["grad"], NF)
    for fr in range(NF):
        alone = bench.value_grad(stage, inp, conf, 1, frames=[fr])
        assert np.array_equal(alone["terms"][0].view(np.uint32), full["terms"][fr].view(np.uint32)), fr
        assert np.array_equal(per_frame_grad(stage, alone["grad"], 1)[0].view(np.uint32), gf[fr].view(np.uint32)), fr
    # and moved: the batch in reverse order gives the reversed rows
    rev = bench.value_grad(stage, inp, conf, NF, frames=np.arange(NF)[::-1])
    assert np.array_equal(rev["terms"][::-1].view(np.uint32), full["terms"].view(np.uint32))
    assert np.array_equal(per_frame_grad(stage, rev["grad"], NF)[::-1].view(np.uint32), gf.view(np.uint32))
    print(f"[smplify {tag}] stage {stage}: each of the {NF} frames alone and the reversed batch: the same bits")


def outputs_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)) for k in ("grad", "terms", "joints", "scalars"))


def check_determinism_and_poison(bench, tag, T=F + 1):
    inp = fixture("value_grad")
    out = {}
    for stage in (1, 2):
        clean = bench.value_grad(stage, inp, conf_of("foot"), T, poison=0)
        again = bench.value_grad(stage, inp, conf_of("foot"), T, poison=0)
        dirty = bench.value_grad(stage, inp, conf_of("foot"), T, poison=0xFF, fill=float("nan"))
        assert outputs_equal(clean, again) and outputs_equal(clean, dirty), stage
        out[stage] = clean
    print(f"[smplify {tag}] two calls, a 0xFF workspace and NaN-filled outputs: the same bits")
    return out


FIT_OUTPUTS = ("pose", "betas", "cam", "joints", "thetas")


def check_fit_repetition_and_poison(bench, tag, T=F + 1):
    """The fit is the call that lives on workspace state (the history ring, ro, H_diag, the gradient pool, prev_flat_grad): two runs
    over a zeroed workspace and one over a 0xFF workspace give the same bits of every output and the same statistics.  A horizon long
    enough for the ring to be read back (several iterations in each of two step() calls per stage)."""
    fx = fixture("fit_short_T%d" % T)
    call = bench.nat.MdmSmplifyCall(num_iters=6, stage1_calls=2, stage2_calls=2)
    runs = [bench.fit(fx["j3d"], conf_of("foot"), call, poison=p) for p in (0, 0, 0xFF)]
    print(f"[smplify {tag}] fit repetition / poison T={T}: evaluations {int(runs[0]['stats'][0])} + {int(runs[0]['stats'][3])}, iterations "
          f"{int(runs[0]['stats'][1])} + {int(runs[0]['stats'][4])}, final loss {runs[0]['stats'][5]:.6e}")
    assert runs[0]["stats"][1] >= 2 and runs[0]["stats"][4] >= 2          # (the history was used)
    for other in runs[1:]:
        for k in FIT_OUTPUTS:
            assert np.isfinite(runs[0][k]).all() and np.array_equal(runs[0][k].view(np.uint32), other[k].view(np.uint32)), k
        assert np.array_equal(runs[0]["stats"], other["stats"])


def check_late_nan_is_reported(bench, tag, T=3):
    """What the first pass does not look at -- the direction, the camera block, cam_est / preserve -- is caught behind the evaluation."""
    base = {k: np.array(v) for k, v in fixture("value_grad").items() if k != "meta"}
    for stage, key in ((1, "dir_cam"), (1, "cam_est"), (2, "dir_body"), (2, "preserve"), (2, "cam")):
        inp = {k: v.copy() for k, v in base.items()}
        inp[key][1, 0] = np.nan
        bench.value_grad(stage, inp, conf_of("ones"), T, expect_rc=-1)
        msg = bench.lib.mdm_last_error().decode()
        assert "not finite" in msg, (stage, key, msg)
    print(f"[smplify {tag}] a NaN in dir, cam_est, preserve or the camera block: reported behind the evaluation ({msg!r})")


def check_nan_is_refused(bench, tag, T=F + 1):
    inp = {k: np.array(v) for k, v in fixture("value_grad").items() if k != "meta"}
    inp["j3d"][T - 2, 7, 1] = np.nan
    for stage in (1, 2):
        got = bench.value_grad(stage, inp, conf_of("ones"), T, fill=-7.0, expect_rc=-1)
        msg = bench.lib.mdm_last_error().decode()
        assert "non-finite" in msg, msg
        assert (got["grad"] == -7.0).all() and (got["terms"] == -7.0).all() and (got["joints"] == -7.0).all() and (got["scalars"] == -7.0).all()
    print(f"[smplify {tag}] a NaN in j3d: refused ({msg!r}), no output written")


def short_call(nat, **over):
    return nat.MdmSmplifyCall(num_iters=4, stage1_calls=1, stage2_calls=1, **over)


def check_short_horizon(bench, T, tag):
    fx = fixture("fit_short_T%d" % T)
    got = bench.fit(fx["j3d"], conf_of("ones"), short_call(bench.nat))
    worst = 0.0
    for k in ("pose", "betas", "cam"):
        dev = float(np.abs(got[k].reshape(-1).astype(np.float64) - fx[k].reshape(-1)).max())
        e_ref = float(fx["e_ref_" + k])
        worst = max(worst, dev / e_ref)
        print(f"[smplify {tag}] short horizon T={T} {k}: deviation {dev:.3e}, e_ref {e_ref:.3e}, ratio {dev / e_ref:.2f}")
    print(f"[smplify {tag}] short horizon T={T} evaluations: step 1 {int(got['stats'][0])}, step 2 {int(got['stats'][3])}; the reference's "
          f"{int(fx['ref_evals'])} in all; final loss {got['stats'][5]:.6e} (reference {float(fx['final_loss']):.6e})")
    for k in ("pose", "betas", "cam"):
        dev = float(np.abs(got[k].reshape(-1).astype(np.float64) - fx[k].reshape(-1)).max())
        assert dev <= FACTOR * float(fx["e_ref_" + k]), (k, dev, float(fx["e_ref_" + k]))
    return got


def rot6d_reference(pose):
    """simplify_loc2rot.py:108-109 on a pose [T, 72] in float64: matrix_to_rotation_6d(axis_angle_to_matrix(.)) -> [T, 24, 6]."""
    R = smh.axis_angle_to_matrix(np.asarray(pose, np.float64).reshape(-1, 24, 3))
    return R[..., :2, :].reshape(R.shape[0], 24, 6)


def check_fit_outputs(got, j3d):
    T = j3d.shape[0]
    assert got["thetas"].shape == (1, 25, 6, T)
    row24 = got["thetas"][0, 24].T                                        # [T, 6]
    assert np.array_equal(row24[:, :3].view(np.uint32), j3d[:, 0].view(np.uint32)) and (row24[:, 3:] == 0).all()
    want = rot6d_reference(got["pose"])
    err = float(np.abs(got["thetas"][0, :24].transpose(2, 0, 1).astype(np.float64) - want).max())
    bound = (3 + 4) * 2.0 ** -24               # entries of a rotation matrix: sums of three products of unit-size terms, in float32
    print(f"[smplify] rot6d of the returned pose: max-abs {err:.3e} (bound {bound:.3e})")
    assert err <= bound, err


def check_whole_fit(bench, T, tag):
    fx = fixture("fit_full_T%d" % T)
    call = bench.nat.MdmSmplifyCall()
    got = bench.fit(fx["j3d"], conf_of("ones"), call)
    loss, ref_loss, spread = float(got["stats"][5]), float(fx["final_loss"]), float(fx["loss_spread"])
    dist = float(np.linalg.norm(got["joints"][:, :22] + got["cam"][:, None] - fx["j3d"], axis=-1).max())
    print(f"[smplify {tag}] whole fit T={T}: final loss {loss:.6e} (reference {ref_loss:.6e}, ensemble spread {spread:.2e}, ratio to the "
          f"reference {loss / ref_loss:.6f}); worst joint-to-target distance {dist * 1e3:.2f} mm (ensemble worst {float(fx['dist_worst']) * 1e3:.2f} mm, "
          f"spread {float(fx['dist_spread']) * 1e3:.3f} mm); evaluations {int(got['stats'][0])} + {int(got['stats'][3])} (reference "
          f"{int(fx['ref_evals_min'])} - {int(fx['ref_evals_max'])}), iterations {int(got['stats'][1])} + {int(got['stats'][4])}")
    assert loss <= ref_loss * (1 + FACTOR * spread), (loss, ref_loss, spread)
    assert dist <= float(fx["dist_worst"]) + FACTOR * float(fx["dist_spread"]), dist
    check_fit_outputs(got, fx["j3d"])
    return got
