"""Batched learned point-mass controllers on the GPU (mppi_create_batch_mlp; k_rollout_mlp2_batch, k_rollout_mlp_small_batch): B
controllers of MPPI_MODEL_MLP, each member with its OWN network, stepped in the same two launches as one.

The contract (include/mppi_c.h): member m is BIT FOR BIT the lone Handle of its config and network on that handle's default kernel -
k_rollout_mlp2 for the [3a, 256, 256, 2a] network, k_rollout_mlp_small for Dense(16); Dense(32) against the handle tuned mlp32_valu = 1 -
fed the same x, goal and sequence on the same step counter. Every comparison with a lone handle is assert_array_equal. One wide and one
narrow member set are also held to the fp64 oracle directly, at the bars DESIGN section 3 states for learned models (costs 2e-5
relative, U' 1e-5); test_batch_mlp_oracle.py proves those cases well conditioned. The case matrix: batch_mlp_util.py."""
import ctypes as C

import numpy as np
import pytest

import batch_mlp_util as N
from batch_util import raw_configs

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


def assert_member_equals_lone(m, hb, i, h, ub, ul, tag):
    msg = "member %d %s" % (i, tag)
    for what in (m.DBG_COSTS, m.DBG_BETA, m.DBG_ETA, m.DBG_U_UPDATED):
        np.testing.assert_array_equal(hb.debug_get(i, what), h.debug_get(what), err_msg=msg)
    np.testing.assert_array_equal(ub[i], ul, err_msg=msg)


def members_equal_lone_handles(m, case, mem, steps=3):
    hb = N.make_batch(m, case, mem)
    assert hb.rollout_kernel_name() == N.kernel_names(case)[0], hb.rollout_kernel_name()
    lone = {i: N.make_lone(m, case, mem, i) for i in N.checked(case)}
    X = mem["X"].copy()
    for step in range(steps):
        ub = hb.next(X)
        assert np.isfinite(ub).all()
        for i, h in lone.items():
            assert_member_equals_lone(m, hb, i, h, ub, h.next(X[i]), "step %d" % step)
        X[:, 0::2] += F32(0.01)  # a new x every step
    Ub = hb.get_action_sequences()
    for i, h in lone.items():
        np.testing.assert_array_equal(Ub[i], h.get_action_sequence())
        h.close()
    assert hb.get_step_counter() == steps
    hb.close()


# ---- 1. member = lone handle, bit for bit -----------------------------------------------------------------------------------------------
CI_1 = N.ids_of(N.WIDE + N.NARROW)


@pytest.mark.parametrize("ci", CI_1, ids=[N.IDS[i] for i in CI_1])
def test_member_equals_its_lone_handle_bit_for_bit(m, ci):
    """three consecutive steps (the warm start shifts, the Philox counter advances): costs, beta, eta, U' and u of every member; the
    members differ in network, normalisation, seed, goal, lambda, gamma, upsilon, sigma and Q"""
    members_equal_lone_handles(m, N.CASES[ci], N.members(ci))


# ---- 2. the tile walk --------------------------------------------------------------------------------------------------------------------
def test_the_tile_walk_of_the_wide_kernel(m):
    """K = 64 (n_cu + 1) + 1: n_cu + 2 tiles per member on n_cu workgroups, so two workgroups of every member own two tiles, and the last
    tile holds one sample"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = dict(id="walk", hid=256, nh=2, a=2, K=64 * (n_cu + 1) + 1, H=2, dense=False, B=2)
    members_equal_lone_handles(m, case, N.build_members(case, 901), steps=2)


# ---- 3. more workgroups than the chip holds --------------------------------------------------------------------------------------------
CI_3 = N.ids_of(N.MANY)


@pytest.mark.parametrize("ci", CI_3, ids=[N.IDS[i] for i in CI_3])
def test_three_hundred_members(m, ci):
    members_equal_lone_handles(m, N.CASES[ci], N.members(ci), steps=2)


# ---- 4. independence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["wide-a2-K65-H5-dense", "dense32x3-a4-K65-H5"])
def test_set_mlp_moves_one_member_and_no_other(m, cid):
    from mppi_tf_amd import _lib as L
    ci = N.INDEX[cid]
    case, mem = N.CASES[ci], N.members(ci)
    other = N.make_net(case, 999)
    a, b = N.make_batch(m, case, mem), N.make_batch(m, case, mem)
    b.set_mlp(1, other)
    ua, ub = a.next(mem["X"]), b.next(mem["X"])
    assert np.abs(ua[1] - ub[1]).max() > 0
    assert np.abs(a.debug_get(1, m.DBG_COSTS) - b.debug_get(1, m.DBG_COSTS)).max() > 0
    for i in (0, 2):
        np.testing.assert_array_equal(ua[i], ub[i])
        for what in (m.DBG_COSTS, m.DBG_BETA, m.DBG_ETA, m.DBG_U_UPDATED):
            np.testing.assert_array_equal(a.debug_get(i, what), b.debug_get(i, what))
    h = N.make_lone(m, case, mem, 1, net=other)  # ... and member 1 is the lone handle of the new network
    np.testing.assert_array_equal(ub[1], h.next(mem["X"][1]))
    np.testing.assert_array_equal(b.debug_get(1, m.DBG_COSTS), h.debug_get(m.DBG_COSTS))
    # another shape: refused, and nothing changes
    wrong = N.make_net(dict(case, hid=16, nh=1), 5)
    with pytest.raises(m.MppiError) as e:
        b.set_mlp(0, wrong)
    assert e.value.status == L.ERR_INVALID_ARG and ("widths" in str(e.value) or "layer count" in str(e.value))
    for bad in (3, -2):
        with pytest.raises(m.MppiError) as e:
            b.set_mlp(bad, other)
        assert e.value.status == L.ERR_INVALID_ARG and "member" in str(e.value)
    a.set_mlp(1, other)  # now a holds b's networks: from the same sequences (the step counters are equal) the two agree in every member
    a.set_action_sequences(mem["U0"])
    b.set_action_sequences(mem["U0"])
    np.testing.assert_array_equal(a.next(mem["X"]), b.next(mem["X"]))
    h.close(), a.close(), b.close()


@pytest.mark.parametrize("cid", ["wide-a2-K65-H5-dense", "dense32x3-a4-K65-H5"])
def test_set_mlp_of_every_member_reaches_all(m, cid):
    ci = N.INDEX[cid]
    case, mem = N.CASES[ci], N.members(ci)
    B = case["B"]
    same = {k: ([v[0]] * B if isinstance(v, list) else np.tile(v[0], (B,) + (1,) * (v.ndim - 1))) for k, v in mem.items()}
    same["nets"] = mem["nets"]
    hb = N.make_batch(m, case, same)
    u = hb.next(same["X"])
    assert np.abs(u[0] - u[1]).max() > 0 and np.abs(u[0] - u[2]).max() > 0  # only their networks differ
    hb.set_mlp(-1, mem["nets"][2])
    hb.set_action_sequences(same["U0"])
    hb.set_step_counter(0)
    u = hb.next(same["X"])
    for i in (1, 2):
        np.testing.assert_array_equal(u[0], u[i])
        np.testing.assert_array_equal(hb.debug_get(0, m.DBG_COSTS), hb.debug_get(i, m.DBG_COSTS))
    hb.close()


# ---- 5. episodes ---------------------------------------------------------------------------------------------------------------------
def _point_mass(m, a, mass=1.0):
    return m.Handle(k=64, tau=4, s_dim=2 * a, a_dim=a, dt=0.1, mass=mass)


@pytest.mark.parametrize("plants", ["own", "shared", "per-member"])
@pytest.mark.parametrize("cid", ["wide-a2-K65-H5-dense", "dense16x3-a4-K65-H5"])
def test_episodes_equal_the_lone_handles_episodes(m, cid, plants):
    """5 steps. As its own plant member m is stepped by its OWN network; on analytic point-mass plants, one shared or one per member,
    by that plant: X, U, C bit for bit the lone handle's episode"""
    from mppi_tf_amd import _lib as L
    ci = N.INDEX[cid]
    case, mem = N.CASES[ci], N.members(ci)
    B, a = case["B"], case["a"]
    hb = N.make_batch(m, case, mem)
    lone = [N.make_lone(m, case, mem, i) for i in range(B)]
    ps = [] if plants == "own" else [_point_mass(m, a)] if plants == "shared" else [_point_mass(m, a, mass) for mass in (0.8, 1.0, 1.3)]
    kb = {} if not ps else dict(plant=ps[0] if len(ps) == 1 else ps)
    Xb, Ub, Cb = hb.run_episode(mem["X"], 5, **kb)
    assert np.isfinite(Xb).all() and np.isfinite(Cb).all()
    for i, h in enumerate(lone):
        kl = {} if not ps else dict(plant=ps[0] if len(ps) == 1 else ps[i])
        Xl, Ul, Cl = h.run_episode(mem["X"][i], 5, **kl)
        msg = "member %d (%s)" % (i, plants)
        np.testing.assert_array_equal(Ub[:, i], Ul, err_msg="U " + msg)
        np.testing.assert_array_equal(Xb[:, i], Xl, err_msg="X " + msg)
        np.testing.assert_array_equal(Cb[:, i], Cl, err_msg="C " + msg)
    assert hb.get_step_counter() == 5
    if plants == "per-member":  # a learned plant stays shared
        learned = [m.Handle(k=64, tau=4, s_dim=2 * a, a_dim=a, mlp=mem["nets"][i]) for i in range(B)]
        with pytest.raises(m.MppiError) as e:
            hb.run_episode(mem["X"], 2, plant=learned)
        assert e.value.status == L.ERR_UNSUPPORTED and "per-member learned plants" in str(e.value)
        ps += learned
    for h in lone + ps:
        h.close()
    hb.close()


# ---- 6. against the oracle, directly ---------------------------------------------------------------------------------------------------
CI_6 = N.ids_of(N.ORACLE)


@pytest.mark.parametrize("ci", CI_6, ids=[N.IDS[i] for i in CI_6])
def test_member_against_the_oracle(m, ci):
    """every member's own noise (debug_get) through the fp64 oracle: costs within 2e-5 relatively, U' within 1e-5"""
    case, mem = N.CASES[ci], N.members(ci)
    hb = N.make_batch(m, case, mem)
    hb.next(mem["X"])
    Ub = hb.get_action_sequences()  # (the shifted U', as the oracle returns it)
    for i in N.checked(case):
        noise = hb.debug_get(i, m.DBG_NOISE)
        np.testing.assert_allclose(noise, N.first_noise(case, mem, i), rtol=0, atol=5e-6)
        ref = N.oracle_step(case, mem, i, mem["U0"][i], noise)
        c = hb.debug_get(i, m.DBG_COSTS).astype(np.float64)
        rel = float((np.abs(c - ref["c64"]) / np.abs(ref["c64"])).max())
        eu = float(np.abs(Ub[i].astype(np.float64) - ref["U64"]).max())
        print("%s member %d: rel cost err GPU %.3g / fp32 CPU %.3g; max|dU'| GPU %.3g / fp32 CPU %.3g" % (
            case["id"], i, rel, ref["rel32"], eu, ref["eu32"]))
        assert rel <= N.COST_BAR, "member %d" % i
        assert eu <= N.U_BAR, "member %d" % i
    hb.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _create(arr, n=None):
    from mppi_tf_amd import _lib
    lib = _lib.load()
    h = _lib._H()
    st = lib.mppi_create_batch_mlp(arr, len(arr) if n is None else n, C.byref(h))
    if h:
        lib.mppi_destroy(h)
    return st, lib.mppi_last_error(None).decode(), bool(h)


def _configs(n, net, a=2, k=128, each_more=None, **fields):
    from mppi_tf_amd import _lib

    def each(i, cfg, keep):
        desc, held = _lib._mlp_desc(net, 3 * a, 2 * a)
        keep += held
        cfg.model_kind, cfg.mlp = _lib.MODEL_MLP, C.pointer(desc)
        for key, v in fields.items():
            setattr(cfg, key, v)
        if each_more:
            each_more(i, cfg, keep)
    return raw_configs(n, 2 * a, a, k=k, tau=4, each=each)


def test_refusals_name_their_cause(m):
    from batch_util import ptr
    from mppi_tf_amd import _lib as L
    lib = L.load()
    narrow = dict(hid=32, nh=2, a=2)
    net = N.make_net(narrow, 1)
    arr, keep = _configs(2, net)
    assert _create(arr)[0] == L.OK
    # MPPI_ERR_UNSUPPORTED, each with the word that names it, and no handle
    unsupported = ((dict(model_kind=L.MODEL_POINT_MASS), "mppi_create_batch_configs"), (dict(model_kind=L.MODEL_AUV), "mppi_create_batch_configs"),
                   (dict(model_kind=L.MODEL_NN_AUV), "mppi_create_batch_learned"), (dict(model_kind=L.MODEL_NN_AUV_SPEED), "mppi_create_batch_learned"),
                   (dict(normalize_cost=1), "normalize_cost"), (dict(flags=2), "MPPI_FLAG_MLP_BF16X3"), (dict(flags=4), "MPPI_FLAG_FP_CONTRACT"),
                   (dict(shard_count=2), "shard_count"), (dict(q_is_full=1), "dense Q"), (dict(state_cost_kind=L.STATE_COST_ELLIPSE), "state cost"))
    for fields, word in unsupported:
        arr, keep = _configs(2, net, **fields)
        st, err, got = _create(arr)
        assert (st, got) == (L.ERR_UNSUPPORTED, False) and word in err, (fields, err)
        assert lib.mppi_last_error(None).decode() == err  # mppi_last_error(NULL) after a failed create
    wide4 = N.make_net(dict(hid=256, nh=2, a=4), 1)
    arr, keep = _configs(2, wide4, a=4)
    st, err, got = _create(arr)
    assert (st, got) == (L.ERR_UNSUPPORTED, False) and "a_dim = 4" in err and "k_rollout_mlp" in err, err
    arr, keep = _configs(1, net, k=64 * 1025)
    st, err, got = _create(arr)
    assert (st, got) == (L.ERR_UNSUPPORTED, False) and "1024 tiles" in err
    arr, keep = _configs(1, net, k=65536)
    assert _create(arr)[0] == L.OK
    # MPPI_ERR_INVALID_ARG
    h = L._H()
    arr, keep = _configs(2, net)
    assert lib.mppi_create_batch_mlp(None, 2, C.byref(h)) == L.ERR_INVALID_ARG and "NULL" in lib.mppi_last_error(None).decode()
    assert lib.mppi_create_batch_mlp(arr, 2, None) == L.ERR_INVALID_ARG
    st, err, _ = _create(arr, 0)
    assert st == L.ERR_INVALID_ARG and "n must be >= 1" in err
    arr[1].mlp = None
    st, err, got = _create(arr)
    assert (st, got) == (L.ERR_INVALID_ARG, False) and "member 1" in err and "cfg.mlp" in err
    # the network's shape and the shared fields: named as batch_shared_diff names them
    a2, k2 = _configs(2, net)
    d2, held2 = L._mlp_desc(N.make_net(dict(narrow, hid=16), 2), 6, 4)
    a2[1].mlp = C.pointer(d2)
    st, err, _ = _create(a2)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].mlp.widths" in err
    d3, held3 = L._mlp_desc(N.make_net(dict(narrow, nh=3), 2), 6, 4)
    a2[1].mlp = C.pointer(d3)
    st, err, _ = _create(a2)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].mlp.n_layers" in err
    d4, held4 = L._mlp_desc(N.make_net(dict(hid=256, nh=2, a=2), 2), 6, 4)  # a wide member in a narrow batch
    a2[1].mlp = C.pointer(d4)
    st, err, _ = _create(a2)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].mlp." in err
    a3, k3 = _configs(2, net)
    a3[1].tau = 5
    st, err, _ = _create(a3)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].tau" in err
    # sigma diagonal for one member, dense for the other
    dense = 0.25 * np.eye(2) + 0.02 * (1 - np.eye(2))
    a4, k4 = _configs(2, net, each_more=lambda i, cfg, kp: setattr(cfg, "sigma", ptr(kp, dense)) if i == 1 else None)
    st, err, got = _create(a4)
    assert (st, got) == (L.ERR_INVALID_ARG, False) and "sigma" in err and "member 1" in err, err


def test_the_other_creators_keep_refusing_the_learned_point_mass(m):
    from batch_util import create_batch_configs
    from mppi_tf_amd import _lib as L
    net = N.make_net(dict(hid=32, nh=2, a=2), 1)
    arr, keep = _configs(2, net)
    st, err, got = create_batch_configs(arr)
    assert (st, got) == (L.ERR_UNSUPPORTED, False) and "model MLP is not supported" in err
    h = L._H()
    assert L.load().mppi_create_batch_learned(arr, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h
    assert "model MLP (the learned point mass) is not supported" in L.load().mppi_last_error(None).decode()
    assert L.load().mppi_create_batch(C.byref(arr[0]), 2, None, C.byref(h)) == L.ERR_UNSUPPORTED and not h


@pytest.mark.parametrize("cid", ["wide-a2-K65-H5-dense", "dense32x3-a4-K65-H5"])
def test_the_handle_refuses_what_a_batch_refuses(m, cid):
    from mppi_tf_amd import _lib as L
    from mppi_tf_amd._lib import fp
    ci = N.INDEX[cid]
    case, mem = N.CASES[ci], N.members(ci)
    a, s = case["a"], 2 * case["a"]
    hb = N.make_batch(m, case, mem)
    lib = hb.lib
    x, u = mem["X"][0].copy(), np.zeros(a, F32)
    assert lib.mppi_next(hb.h, fp(x), s, fp(u), a) == L.ERR_UNSUPPORTED and "mppi_batch_" in lib.mppi_last_error(hb.h).decode()
    desc, held = L._mlp_desc(mem["nets"][0], 3 * a, s)
    assert lib.mppi_set_mlp(hb.h, C.byref(desc)) == L.ERR_UNSUPPORTED and "mppi_batch_set_mlp" in lib.mppi_last_error(hb.h).decode()
    assert lib.mppi_set_goal(hb.h, fp(x), s) == L.ERR_UNSUPPORTED
    assert lib.mppi_set_sequence_filter(hb.h, 5, 3) == L.ERR_UNSUPPORTED and "mppi_set_sequence_filter" in lib.mppi_last_error(hb.h).decode()
    assert lib.mppi_set_transition_log(hb.h, 8) == L.ERR_UNSUPPORTED and "mppi_set_transition_log" in lib.mppi_last_error(hb.h).decode()
    for key in ("mlp32_valu", "mlp_v1", "fused_step", "prelaunch", "force_tile_kernel"):
        with pytest.raises(m.MppiError) as e:
            hb.set_tuning(key, 1)
        assert e.value.status == L.ERR_UNSUPPORTED and key in str(e.value)
    # what serves any batch serves this one
    hb.set_action_limits([-0.01] * a, [0.01] * a)
    ul = hb.next(mem["X"])
    assert np.abs(hb.get_action_sequences()).max() <= F32(0.01) and np.abs(ul).max() <= F32(0.01)
    hb.set_goals(mem["G"][::-1])
    hb.set_step_counter(7)
    assert hb.get_step_counter() == 7
    hb.profile_begin(2)
    hb.next(mem["X"])
    r, f, n = hb.profile_end()
    assert n == 1 and r > 0 and f > 0
    hb.close()


def test_next_device_on_a_torch_stream_equals_next(m):
    import torch
    ci = N.INDEX["wide-a3-K65-H5-diag"]
    case, mem = N.CASES[ci], N.members(ci)
    a, b = N.make_batch(m, case, mem), N.make_batch(m, case, mem)
    st = torch.cuda.Stream()
    xd, ud = torch.tensor(mem["X"], device="cuda"), torch.zeros(case["B"], case["a"], device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        b.next_device(xd.data_ptr(), ud.data_ptr(), st)
        st.synchronize()
        np.testing.assert_array_equal(ud.cpu().numpy(), a.next(mem["X"]))
    a.close(), b.close()


# ---- 8. the learner bridge ------------------------------------------------------------------------------------------------------------
def _trained(m, hidden, B=3, a=2, seed=3):
    """(the model, a B-member learner batch after 2 Adam steps at B rates, its class)"""
    s = 2 * a
    rng = np.random.default_rng(seed)
    model = m.NNPointMassModel(stateDim=s, actionDim=a, hidden=hidden, seed=seed)
    model.set_Xmean_Xstd(rng.uniform(-0.1, 0.1, 3 * a), rng.uniform(0.8, 1.2, 3 * a))
    model.set_Ymean_Ystd(rng.uniform(-0.01, 0.01, s), rng.uniform(0.8, 1.2, s))
    w = model.get_weights()
    cls = m.WideLearnerBatch if hidden == (256, 256) else m.LearnerBatch
    lb = cls(dict(W=w[0::2], b=w[1::2]), B)
    n = 96
    lb.set_data(rng.standard_normal((n, 3 * a)).astype(F32), (0.1 * rng.standard_normal((n, s))).astype(F32))
    for i in range(B):
        lb.set_split(i, np.arange(i, n, 2), None)
    lb.train(2, np.array([1e-3, 1e-2, 3e-2], F32)[:B])
    return model, lb


@pytest.mark.parametrize("hidden", [(32, 32), (256, 256)], ids=["narrow", "wide"])
def test_load_learners_and_episode_fold(m, hidden):
    """a 3-member LearnerBatch (hidden 32) / WideLearnerBatch after 2 Adam steps -> the controllers; episode_fold's C.sum(0) equals lone
    controllers loaded with get_weights(m)"""
    a, s, B, K, H, steps = 2, 4, 3, 65, 5, 3
    model, lb = _trained(m, hidden)
    task = dict(k=K, tau=H, dt=0.1, lam=0.9, sigma=0.3 * np.eye(a, dtype=F32), goal=np.array([1.0, 0.0, -1.0, 0.0], F32), Q=np.array([10.0, 1.0, 10.0, 1.0], F32))
    seeds = [3, 4, 5]
    ctl = m.BatchHandle.learned(B, model.mlp(), "mlp", a_dim=a, seeds=seeds, **task)
    ctl.load_learners(lb, model)
    x0 = np.array([0.1, 0.0, -0.2, 0.1], F32)
    X = np.tile(x0, (B, 1))
    u = ctl.next(X)
    nets = [dict(lb.get_weights(i), **model.normalisation()) for i in range(B)]
    tuned = {"mlp32_valu": 1} if hidden[0] == 32 else None
    lone = [m.Handle(s_dim=s, a_dim=a, seed=seeds[i], mlp=nets[i], tuning=tuned, **task) for i in range(B)]
    for i, h in enumerate(lone):
        np.testing.assert_array_equal(u[i], h.next(x0), err_msg="member %d" % i)
    assert np.abs(u[0] - u[2]).max() > 0  # the rates differ, so do the networks
    plant = _point_mass(m, a)
    cost = m.LearnerBase(model).episode_fold(lb, ctl, plant, x0, steps)
    assert cost.shape == (B,) and np.isfinite(cost).all()
    for i, h in enumerate(lone):
        h.set_action_sequence(np.zeros((H, a), F32))
        h.set_step_counter(0)
        Cl = h.run_episode(x0, steps, plant=plant)[2]
        np.testing.assert_array_equal(cost[i], Cl.sum(0), err_msg="member %d" % i)
        h.close()
    ctl.close(), plant.close(), lb.close()


def test_grid_search_by_episode_on_a_narrow_point_mass_model(m):
    a, s, K, H, k, steps = 2, 4, 64, 4, 2, 3
    rates = [1e-3, 3e-2]
    rng = np.random.default_rng(5)
    model = m.NNPointMassModel(stateDim=s, actionDim=a, hidden=(32, 32), seed=2)
    learner = m.LearnerBase(model, bufferSize=40)
    plant = _point_mass(m, a)
    x = (0.3 * rng.standard_normal((40, s))).astype(F32)
    v = (0.5 * rng.standard_normal((40, a))).astype(F32)
    learner.add_rb(x[:, :, None], v[:, :, None], plant.model_next(x, v)[:, :, None])
    learner.stats()
    task = dict(k=K, tau=H, dt=0.1, sigma=0.5 * np.eye(a, dtype=F32), goal=np.array([1.0, 0.0, -1.0, 0.0], F32), Q=np.array([10.0, 1.0, 10.0, 1.0], F32))
    ctl = m.BatchHandle.learned(len(rates) * k, model.mlp(), "mlp", a_dim=a, seeds=[1] * (len(rates) * k), **task)
    episode = dict(controller=ctl, plant=plant, x0=np.zeros(s, F32), n_steps=steps)
    best, table = learner.grid_search(rates, k=k, epoch=3, by="episode", episode=episode)
    log = learner.kfold_log["episode"]
    assert log.shape == (1, len(rates), k) and np.isfinite(log).all()
    np.testing.assert_array_equal(table, log[-1].astype(np.float64).mean(axis=1))
    assert best == rates[int(np.argmin(table))]
    # k_fold_validation(episode=) is the same table
    log2 = learner.k_fold_validation(k=k, learningRate=rates, epoch=3, episode=episode)["episode"]
    np.testing.assert_array_equal(log2, log)
    ctl.close(), plant.close()


def test_learn_loop_ranks_point_mass_rates_by_an_episode(m, capsys):
    """examples/learn_loop.py --model point_mass --hidden 32 --kfold K --lrs a,b --kfold-episode: a line per round with the episode table,
    whose argmin trains the round; the wide network's folds have no episode harness and the example says so"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    argv = ["--model", "point_mass", "--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "12", "--epochs", "3", "--layers", "2",
            "--kfold", "2", "--lrs", "1e-3,1e-2", "--kfold-episode", "--episode-steps", "3"]
    _, _, figures = learn_loop.main(argv + ["--hidden", "32"])
    out = capsys.readouterr().out.splitlines()
    tables = [l for l in out if "summed state cost of a 3-step closed-loop episode" in l]
    assert len(tables) == 2 and all("-> lr 0.01" in l or "-> lr 0.001" in l for l in tables), out
    for l in tables:  # the chosen rate is the argmin of the printed table
        cells = dict(c.split(": ") for c in l.split("by learning rate: ")[1].split(" -> lr ")[0].split(", "))
        best = min(cells, key=lambda r: float(cells[r]))
        assert float(l.split("-> lr ")[1]) == float(best), l
    assert np.isfinite(np.array([f[:5] for f in figures])).all()
    with pytest.raises(SystemExit):
        learn_loop.main(argv + ["--hidden", "256"])
    assert "--hidden 256" in capsys.readouterr().err
