"""mdm_amd/evaluator.py on the MI355X: every fixture of tests/golden/evaluator_*.npz under the accuracy condition, batch sizes and
frame counts around every tile edge against the fp64 restatement, row invariance, KIT's input width, R-precision's boolean matrix, and a
call on a side stream behind a sampler loop.

Accuracy condition: max-abs error against fp64 <= 4 x e_ref, e_ref = the reference's own fp32 error on that fixture
(PIN_REPORT_evaluator.json).  Cases without a fixture of their own take the e_ref of the full-width motion fixture with the same kind
of weights (same widths, same depth of sums, at most as many steps), named at each use.

Every test prints its figure before it asserts; tools/bench_evaluator.py collects them into profiles/r09a_evaluator.md."""
import numpy as np
import pytest
import torch

import evaluator_helpers as eh
from helpers import maxabs, memo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _bound(name):
    return 4 * eh.pin_report()[name]["e_ref"]


def _wrapper(name):
    return memo(("eval_wrapper", name), lambda: eh.make_wrapper(name, eh.fixture_weights(name), DEV))


def _full_wrapper(trained=True, dims=None, dataset="humanml"):
    key = ("eval_full", trained, dataset)
    weights = memo(key + ("w",), lambda: eh.build_weights(31, dims or eh.FULL, trained))
    return memo(key, lambda: eh.make_wrapper(dims or eh.FULL, weights, DEV, dataset_name=dataset)), weights


@pytest.mark.parametrize("name", list(eh.FIXTURES))
def test_fixture_meets_the_accuracy_condition(name):
    f, inp, g = eh.FIXTURES[name], eh.fixture_inputs(name), eh.load_fixture(name)
    w = _wrapper(name)
    got = {}
    if f["kind"] == "motion":
        got["motion"] = w.get_motion_embeddings(_t(inp["motions"]), _t(inp["m_lens"]))
    elif f["kind"] == "text":
        got["text"] = w._text_rows(_t(inp["word_embs"]).to(DEV), _t(inp["pos_ohot"]).to(DEV), inp["cap_lens"].tolist())
    else:
        got["text"], got["motion"] = w.get_co_embeddings(_t(inp["word_embs"]), _t(inp["pos_ohot"]), _t(inp["cap_lens"]),
                                                         _t(inp["motions"]), _t(inp["m_lens"]))
    bound = _bound(name)
    for k, v in got.items():
        err = maxabs(v.cpu(), g[f"fp64_{k}"])
        print(f"[evaluator] {name} {k}: max-abs vs fp64 = {err:.3e}  e_ref = {bound / 4:.3e}  bound = {bound:.3e}")
    for k, v in got.items():
        assert v.shape == g[f"fp64_{k}"].shape and bool(torch.isfinite(v).all())
        assert maxabs(v.cpu(), g[f"fp64_{k}"]) <= bound
    if f["kind"] == "co":
        # metrics.calculate_R_precision's boolean matrix: identical on the GPU embeddings and on the reference's (the generator checked
        # that the nearest distances are more than 100 x e_ref apart, so rounding does not decide the ranking)
        assert eh.pin_report()[name]["nearest_distance_gap"] > 100 * eh.pin_report()[name]["e_ref"]
        mine = eh.top_k_matrix(got["text"].cpu().numpy(), got["motion"].cpu().numpy())
        assert np.array_equal(mine, eh.top_k_matrix(g["ref_text"], g["ref_motion"]))


def _batch64():
    """64 motions of T = 196, lengths distinct and descending (so the wrapper's reordering is the identity), and their fp64 result."""
    w, weights = _full_wrapper(trained=True)
    m_lens = [196 - 2 * i for i in range(64)]
    motions = eh.make_motion_inputs(32, 64, 196, 263, m_lens)
    want = memo(("eval_batch64", "fp64"), lambda: eh.motion_embeddings_fp64(weights, motions, m_lens)[0])
    return w, motions, m_lens, want


@pytest.mark.parametrize("B", [1, 3, 32, 33, 64])
def test_batch_sizes_at_full_width(B):
    w, motions, m_lens, want = _batch64()
    got = w.get_motion_embeddings(_t(motions[:B]), torch.tensor(m_lens[:B]))
    err = maxabs(got.cpu(), want[:B])
    print(f"[evaluator] B={B} T=196: max-abs vs fp64 = {err:.3e} (bound {_bound('motion_b32_full_trained'):.3e})")
    assert got.shape == (B, 512) and err <= _bound("motion_b32_full_trained")


def test_row_invariance_is_bit_exact():
    """One (motion, length) pair alone, inside a batch of 32 with mixed lengths, and in two calls: the same bits."""
    w, motions, m_lens, _ = _batch64()
    row = 5
    alone = w.get_motion_embeddings(_t(motions[row:row + 1]), torch.tensor(m_lens[row:row + 1]))
    again = w.get_motion_embeddings(_t(motions[row:row + 1]), torch.tensor(m_lens[row:row + 1]))
    idx = [row] + [i for i in range(40) if i != row][:31]          # lengths 196 .. 118, the row somewhere in the middle after sorting
    lens = [m_lens[i] for i in idx]
    batch = w.get_motion_embeddings(_t(motions[idx]), torch.tensor(lens))
    pos = list(np.argsort(lens)[::-1]).index(0)
    assert torch.equal(alone, again)
    assert torch.equal(alone[0], batch[pos])


@pytest.mark.parametrize("T", [4, 6, 40, 197])
def test_frame_counts_around_the_conv_floor(T):
    w, weights = _full_wrapper(trained=True)
    m_lens = [T, max(4, T - 3), max(4, T // 2)]
    motions = eh.make_motion_inputs(40 + T, 3, T, 263, m_lens)
    got = w.get_motion_embeddings(_t(motions), torch.tensor(m_lens))
    want, _ = eh.motion_embeddings_fp64(weights, motions, m_lens)
    err = maxabs(got.cpu(), want)
    print(f"[evaluator] T={T}: max-abs vs fp64 = {err:.3e} (bound {_bound('motion_b32_full_trained'):.3e})")
    assert err <= _bound("motion_b32_full_trained")


def test_kit_input_width():
    dims = dict(eh.FULL, dim_pose=251)
    w, weights = _full_wrapper(trained=False, dims=dims, dataset="kit")
    assert w.opt["dim_pose"] == 251
    m_lens = [120, 64, 33]
    motions = eh.make_motion_inputs(50, 3, 120, 251, m_lens)
    got = w.get_motion_embeddings(_t(motions), torch.tensor(m_lens))
    want, _ = eh.motion_embeddings_fp64(weights, motions, m_lens)
    err = maxabs(got.cpu(), want)
    print(f"[evaluator] KIT 251 features: max-abs vs fp64 = {err:.3e} (bound {_bound('motion_b32_full_default'):.3e})")
    assert err <= _bound("motion_b32_full_default")


def test_call_on_a_side_stream_behind_a_sampler_loop():
    """One chain per device (include/mdm_hip.h CONCURRENCY): an evaluator call on a non-default stream right behind a sampling loop on
    the default stream is ordered behind it and returns what the same call returns on the default stream."""
    from helpers import make_pair, small_state_dict, synth_y
    w, motions, m_lens, _ = _batch64()
    base = w.get_motion_embeddings(_t(motions[:8]), torch.tensor(m_lens[:8]))
    model, diffusion = make_pair(small_state_dict(), 4, DEV)
    y = synth_y(2, 24, seed=1, lengths=[24, 17])
    y = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in y.items()}
    sample = diffusion.p_sample_loop(model, (2, 263, 1, 24), clip_denoised=False, model_kwargs={"y": y})
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = w.get_motion_embeddings(_t(motions[:8]), torch.tensor(m_lens[:8]))
    side.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sample).all())
    assert torch.equal(got, base)
