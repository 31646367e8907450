"""The tail of the pose stage (csrc/pose_chain.hip on csrc/pose_device.h) against its numpy twin tests/_pose_ref.py, byte for
byte: svo_chain_relative at the chain's staging bounds (64 pairs a trip), and the step records of svo_add_frame and
svo_track_batch over one short sequence -- T_rel_inv = inv_rt(R, tvec), pose = mul4(previous pose, T_rel_inv), the cleared
record of a failed pair.  Both sides do the same float64 operations in the same order, so nothing here has a tolerance."""
import numpy as np
import pytest

import _pose_ref as PR

pytestmark = pytest.mark.gpu

N_SYNTH = 9                              # the frames of tests/test_gpu_window.py; one blank frame follows, so the last pair fails


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def chain_cases():
    """(n, seeded) -> (T, ok, pose0, the twin's poses), computed once"""
    return {k: c + (PR.chain(*c),) for k, c in PR.chain_cases().items()}


@pytest.fixture(scope="module")
def chain_ctx(pkg):
    c = pkg.Context(64, 64, device=0)
    yield c
    c.close()


@pytest.mark.parametrize("seeded", [False, True], ids=["identity", "pose0"])
@pytest.mark.parametrize("n", PR.CHAIN_N)
def test_chain_relative_equals_the_twin(tc, chain_ctx, chain_cases, n, seeded):
    T, ok, pose0, want = chain_cases[n, seeded]
    host = chain_ctx.chain_relative(T.reshape(n, 16), ok, pose0)
    assert host.tobytes() == want.tobytes(), "HOST"
    dev = chain_ctx.chain_relative(tc.from_numpy(T.reshape(n, 16)).cuda(), tc.from_numpy(ok).cuda(), pose0)
    chain_ctx.sync()
    assert dev.cpu().numpy().tobytes() == want.tobytes(), "DEVICE"


# ---- the step records of the fused paths
@pytest.fixture(scope="module")
def frames10(synth, tc):
    from test_gpu_ingest import _render
    seq, frames = _render(synth, tc, 416, 128, N_SYNTH)
    return seq, list(frames) + [(np.zeros_like(frames[0][0]), np.zeros_like(frames[0][0]))]


@pytest.fixture(scope="module")
def online_records(pkg, frames10):
    """the records of svo_add_frame over the ten frames, the init record included"""
    seq, frames = frames10
    c = pkg.Context(416, 128, device=0, P1=seq.proj()[0], P2=seq.proj()[1])
    recs = [c.add_frame(L, R)[1] for L, R in frames]
    c.close()
    return recs


def _cleared(pkg, **fields):
    """the cleared step record -- counts 0, R = I, T_rel_inv = I, pose 0 -- with `fields` filled in"""
    r = np.zeros((), pkg.STEP_DTYPE)
    r["R"] = np.eye(3).reshape(9)
    r["T_rel_inv"] = np.eye(4).reshape(16)
    for k, v in fields.items():
        r[k] = v
    return r


def test_online_records_follow_the_twin(pkg, online_records):
    recs = online_records
    first = recs[0]
    assert first.tobytes() == _cleared(pkg, ok=1, n_cur_kps=first["n_cur_kps"], pose=np.eye(4).reshape(16)).tobytes(), "the init record"
    assert [int(r["ok"]) for r in recs[1:-1]].count(1) >= N_SYNTH // 2 and int(recs[-1]["ok"]) == 0       # a condition on the inputs
    pose = first["pose"].reshape(4, 4)
    for f, r in enumerate(recs[1:], 1):
        if int(r["ok"]):
            assert int(r["fail_stage"]) == 0
            Ti = PR.inv_rt(r["R"], r["tvec"])
            assert r["T_rel_inv"].tobytes() == Ti.tobytes(), "T_rel_inv of frame %d" % f
            pose = PR.mul4(pose, Ti)
        assert r["pose"].tobytes() == pose.tobytes(), "pose of frame %d" % f
    last = recs[-1]                                       # the blank frame: no corners, nothing tracked or solved
    assert int(last["fail_stage"]) != 0 and int(last["n_cur_kps"]) == 0
    want = _cleared(pkg, fail_stage=last["fail_stage"], n_prev_kps=last["n_prev_kps"], n_cur_kps=last["n_cur_kps"], n_tracked=last["n_tracked"],
                    pose=recs[-2]["pose"])
    assert last.tobytes() == want.tobytes(), "the failed pair's record"


def test_batch_records_equal_the_online_ones(pkg, tc, frames10, online_records):
    seq, frames = frames10
    c = pkg.Context(416, 128, device=0, P1=seq.proj()[0], P2=seq.proj()[1], max_batch=16)
    L = tc.from_numpy(np.stack([f[0] for f in frames])).cuda()
    R = tc.from_numpy(np.stack([f[1] for f in frames])).cuda()
    got = c.track_batch(L, R)
    c.close()
    assert len(got) == len(frames) - 1
    for p, (g, w) in enumerate(zip(got, online_records[1:])):
        assert g.tobytes() == w.tobytes(), "pair %d" % p
