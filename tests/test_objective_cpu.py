"""The host route of blindshadowremoval_amd/objective.py against the three host statements composed here, at S = 32, B = 2, without a
generator: the total gradient's addition order bit for bit, grad_gs, the totals of the route's losses, and the tail norms.  Then the
table of the backward pass: its host walk over all five stages against the five statements called by hand, and its refusals."""
import numpy as np
import pytest

from blindshadowremoval_amd import discriminator, generator_grad, objective, perceptual, train_losses
from blindshadowremoval_amd.weights import init_discriminator_weights, init_vgg_weights

import clr_tail_grad_cases

f32 = np.float32
SEED = 1          # train_losses.example_inputs(32, 2, SEED): an input on which the three orders of adding the terms give different bytes (asserted below)


@pytest.fixture(scope="module")
def route():
    return objective.HostRoute(init_discriminator_weights(1), init_vgg_weights(21), clr_tail_grad_cases.tail_weights())


@pytest.fixture(scope="module")
def arrays():
    return train_losses.example_inputs(32, 2, SEED)


@pytest.fixture(scope="module")
def statements(route, arrays):
    """The three statements' results on the inputs, computed once."""
    img, gt, mask_sv, gs, con_rgb = arrays
    return (train_losses.step_losses_grad(*arrays, upstream=np.array(train_losses.G_TOTAL_WEIGHTS, f32)),
            discriminator.gen_grad(route.disc_w, gt, con_rgb, mask_sv), discriminator.gan_losses(route.disc_w, gt, con_rgb, mask_sv),
            perceptual.per_loss_grad(route.vgg_w, gt, con_rgb, upstream=objective.PER_WEIGHT))


@pytest.fixture(scope="module")
def total(route, arrays):
    return route.total_grad(*arrays)


def test_total_gradient_is_the_three_terms_added_in_the_stated_order(total, statements):
    three, gen, _, per = statements
    a, b, c = three["grad_con"], gen["grad"].astype(f32), per["grad"]
    assert a.dtype == b.dtype == c.dtype == f32 and objective.PER_WEIGHT == f32(.005)
    grad_con = total[3]
    assert grad_con.dtype == f32 and grad_con.shape == (2, 32, 32, 3)
    assert grad_con.tobytes() == ((a + b) + c).tobytes()
    for other in (a + (b + c), (a + c) + b):
        assert grad_con.tobytes() != other.tobytes()


def test_grad_gs_is_step_losses_grads_own(total, statements):
    assert total[4].tobytes() == statements[0]["grad_gs"].tobytes() and np.abs(total[4]).max() > 0


def test_totals_of_the_routes_losses(route, arrays, total, statements):
    three, _, gan, per = statements
    want_g = objective.g_total_loss(three["losses"][0], three["losses"][1], three["losses"][2], gan["losses"][0], per["loss"][0])
    want_d = objective.d_total_loss(gan["losses"][1], gan["losses"][2])
    for got in (total[:3], route.losses(*arrays)[:3], route.losses(*arrays, per_grad=True)[:3]):
        record = objective.loss_record(*got)
        assert tuple(record) == objective.ALL_NAMES
        assert f32(record["g_total"]).tobytes() == want_g.tobytes() and f32(record["d_total"]).tobytes() == want_d.tobytes()
        assert [f32(record[k]) for k in objective.LOGGED] == list(three["losses"]) + list(gan["losses"]) and f32(record["per"]) == per["loss"][0]
    assert route.losses(*arrays)[3] is None
    assert route.losses(*arrays, per_grad=True)[3].tobytes() == per["grad"].tobytes()


def test_tail_norms_are_those_of_tail_grad_on_the_same_gradients(route, arrays, total):
    gs = arrays[3]
    f = generator_grad.example_inputs(32, 32, 2, 4)[1]
    assert f.shape == (2, 32, 32, 64)
    tail_route = objective.HostRoute(route.disc_w, route.vgg_w, route.gen_w, wanted=("tail",))
    got = tail_route.stage_norms(dict(img=arrays[0], gs=gs, mask22=None, grad_con=total[3], grad_gs=total[4]), {"f": f})["tail"]
    want = generator_grad.tail_norms(generator_grad.tail_grad(route.gen_w, gs, f, total[3], total[4]))
    assert len(got) == len(objective.tail_grad_names()) == 24
    assert got == [v for name in generator_grad.TAIL_NORM_NAMES for v in want[name]] and all(v > 0 for v in got)


# ---- the table of the backward pass and its host walk, at (H, W, B) = (16, 32, 2): a coarse grid of 2 x 4 and an image seam
ALL_STAGES = ("tail", "decoder", "nonlocal", "bottleneck", "heads")


@pytest.fixture(scope="module")
def walked(route):
    """The context and every probe as seeded arrays -> (context, probes, the host walk's results with all five stages wanted)."""
    H, W, B = 16, 32, 2
    gs, f, grad_con, grad_gs = generator_grad.example_inputs(H, W, B, 5)
    img, y, _ = generator_grad.heads_example_inputs(H, W, B, 5)
    rng = np.random.default_rng(77)

    def kept(h, w, c):                   # like a LeakyReLU output, as the forward's kept tensors are
        a = rng.standard_normal((B, h, w, c)).astype(f32)
        return np.where(a >= 0, a, f32(.3) * a).astype(f32)

    context = dict(img=img, gs=gs, mask22=rng.uniform(0, 1, (B, H, W, 3)).astype(f32), grad_con=grad_con, grad_gs=grad_gs)
    probes = dict(f=f, y=y, f2=kept(H // 2, W // 2, 96), f1=kept(H // 4, W // 4, 128), res5=kept(H // 8, W // 8, 261),
                  res4=kept(H // 8, W // 8, 261), y3x5=rng.standard_normal((B, H // 8, W // 8, 261)).astype(f32))
    return context, probes, objective.host_walk(ALL_STAGES, route.gen_w, context, probes)


def test_table_states_the_stages_their_parents_and_what_they_hand_on():
    assert tuple(s.name for s in objective.BACKWARD) == ALL_STAGES
    assert [s.parent for s in objective.BACKWARD] == [None, "tail", "decoder", "nonlocal", "tail"]
    assert [s.gives for s in objective.BACKWARD] == [("d_f", "d_gs"), ("d_x",), ("d_y3", "d_skip"), ("d_xin",), ("d_y",)]
    assert [s.takes for s in objective.BACKWARD] == [("gs", "grad_con", "grad_gs"), ("d_f",), ("d_x",), ("d_y3", "d_skip"), ("img", "mask22", "d_gs")]
    assert objective.STAGES == ALL_STAGES[:4]


def test_host_walk_is_the_five_statements_called_by_hand(route, walked):
    """Byte for byte: every gradient of every stage, then the route's norm lists and their order against stage_grad_names."""
    context, p, got = walked
    w, c, host = route.gen_w, context, generator_grad
    t = host.tail_grad(w, c["gs"], p["f"], c["grad_con"], c["grad_gs"])
    acts = {k: p[k] for k in ("res5", "f1", "f2", "f")}
    d = host.decoder_grad(w, acts["res5"], t["d_f"], acts=acts)
    xin = p["res4"]
    y3 = (p["y3x5"][..., :257] - xin[..., :257]).astype(f32)
    n = host.nonlocal_grad(w, y3, xin, d["d_x"], acts={"out": acts["res5"]})
    b = host.bottleneck_grad(w, p["res4"], n["d_y3"], n["d_skip"])
    mask = (c["mask22"][..., 0:1] - c["mask22"][..., 2:3]).astype(f32)
    h = host.heads_grad(w, c["img"], p["y"], t["d_gs"].astype(f32), acts={"mask": mask})
    want = dict(zip(ALL_STAGES, (t, d, n, b, h)))
    assert tuple(got) == ALL_STAGES
    for stage in ALL_STAGES:
        assert set(got[stage]) == set(want[stage]), stage
        for k, v in want[stage].items():
            assert np.asarray(got[stage][k]).dtype == np.asarray(v).dtype and np.asarray(got[stage][k]).tobytes() == np.asarray(v).tobytes(), (stage, k)
    walking = objective.HostRoute(route.disc_w, route.vgg_w, w, wanted=ALL_STAGES)
    lists = walking.stage_norms(context, p)
    assert tuple(lists) == ALL_STAGES
    for stage in ALL_STAGES:
        names = getattr(host, stage.upper() + "_NORM_NAMES")
        norms = getattr(host, stage + "_norms")(want[stage])
        assert lists[stage] == [v for pair in norms.values() for v in pair] == [v for name in names for v in norms[name]], stage
        assert objective.stage_grad_names(stage) == [name + s for name in names for s in ("_l1", "_linf")] and len(lists[stage]) == 2 * len(names)
        assert all(np.abs(want[stage][name]).max() > 0 for name in names), stage        # nothing above passes on zeros


REFUSALS = {"tail": "--tail goes with --grad-total", "decoder": "--decoder goes with --grad-total --tail",
            "nonlocal": "--nonlocal goes with --grad-total --tail --decoder",
            "bottleneck": "--bottleneck goes with --grad-total --tail --decoder --nonlocal", "heads": "--heads goes with --grad-total --tail"}


def test_a_stage_is_refused_without_its_parent_and_not_with_it(capsys):
    """The parent of `tail` is --grad-total itself."""
    rows = {s.name: s for s in objective.BACKWARD}
    for s in objective.BACKWARD:
        above, parent = [], s.parent               # the stage's ancestors, the root first
        while parent is not None:
            above.insert(0, parent)
            parent = rows[parent].parent
        without = [s.name] + above[:-1]
        assert objective.refusal([s.name] + above, True) is None
        assert objective.refusal(without, bool(above)) == REFUSALS[s.name]
        flags = {rows[a].dest: True for a in without}
        with pytest.raises(ValueError, match="^perceptual: %s$" % REFUSALS[s.name]):
            objective.score_folder("no folder", "no.npz", grad_total=bool(above), **flags)
        with pytest.raises(SystemExit):
            objective.main(["no folder", "--vgg", "no.npz"] + ["--grad-total"] * bool(above) + ["--" + a for a in without])
        assert capsys.readouterr().err.strip().endswith("error: " + REFUSALS[s.name])
