"""The gradient hand-off protocols of layers/handoff.py, driven on the CPU in
every arrival order (the full-model GPU tests see only the order autograd
happens to pick).  A stand-in replaces the conv backward's one _dgrad call: it
returns a given tensor and records the add / add2 / gate it was asked for."""
import pytest
import torch

from detectron2_tensorflow_amd.layers import handoff as H
from detectron2_tensorflow_amd.layers.conv_grad import input_grad
from detectron2_tensorflow_amd.layers.handoff import (DeferredPixels, HandoffError,
                                                      LevelAccumulator, Links, Pair, PoolerShare,
                                                      ReluTag, Slot)

SHAPE = (2, 4, 5, 8)


def rnd(seed):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(seed))


class _Body(torch.autograd.Function):
    """A CPU autograd node whose backward runs ``fn`` (deposits queue their
    completion checks on the engine, so they need a real backward pass)."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def in_backward(*fns):
    """One backward pass that reaches a node per fn, in the order given."""
    x = torch.zeros(1, requires_grad=True)
    # (ready nodes run newest first)
    sum(_Body.apply(x, fn) for fn in reversed(fns)).sum().backward()
    return x


def conv_backward(links, gx, gate_ok=True):
    """_ConvMFMAFn.backward's input-gradient step with the dgrad stood in:
    (what the backward returns for x, what the dgrad was asked for)."""
    asked = {}

    def dgrad(gate, add, add2):
        asked.update(add=add, add2=add2, gate=gate)
        return gx

    return input_grad(links, gate_ok, dgrad), asked


def bound(links, x=None, topdown=None, has_residual=False):
    links.bind(torch.zeros(1) if x is None else x, topdown, has_residual)
    return links


def relu_output():
    x, tag = torch.zeros(1), ReluTag()
    H.tag(x, H.RELU, tag)
    return x, tag


class FakePixels(DeferredPixels):
    """A DeferredPixels whose pass adds a known map."""
    __slots__ = ("pooled", "runs")

    def __init__(self, pooled):
        self.pooled, self.runs = pooled, []

        def run(level, m, accumulate):
            self.runs.append("add_into" if accumulate else "materialize")
            if accumulate:
                m += pooled
            else:
                m.copy_(pooled)

        super().__init__(run, 2, pooled.shape, pooled.device)


# ------------------------------------------------------------------- Pair
@pytest.mark.parametrize("swap", [False, True])
def test_pair_first_deposits_second_adds(swap):
    pair = Pair()
    a, b = bound(Links(pair=pair)), bound(Links(pair=pair))
    first, second = (b, a) if swap else (a, b)
    g1, g2 = rnd(1), rnd(2)
    out = {}

    def body():
        out["first"] = conv_backward(first, g1)
        assert pair.g is g1 and not pair.empty
        out["second"] = conv_backward(second, g2)

    in_backward(body)
    assert out["first"] == (None, {"add": None, "add2": None, "gate": False})
    got, asked = out["second"]
    assert got is g2 and asked["add"] is g1 and asked["add2"] is None and not asked["gate"]
    assert pair.empty


def test_pair_with_residual_link_adds_link_plus_other():
    pair, link = Pair(), Slot()
    x, tag = relu_output()
    first = bound(Links(pair=pair))
    second = bound(Links(sole_consumer=True, grad_from=link, pair=pair), x)
    gl, g1, g2 = rnd(3), rnd(4), rnd(5)
    out = {}

    def body():
        link.put(gl)
        conv_backward(first, g1)
        out["second"] = conv_backward(second, g2)

    in_backward(body)
    got, asked = out["second"]
    assert got is g2 and asked["gate"] and tag.masked
    assert torch.equal(asked["add"], gl + g1)
    assert link.empty and pair.empty


def test_first_of_a_pair_is_neither_gated_nor_marked_but_adds_its_link():
    pair, link = Pair(), Slot()
    x, tag = relu_output()
    first = bound(Links(sole_consumer=True, grad_from=link, pair=pair), x)
    gl, g1 = rnd(6), rnd(7)
    out = {}

    def body():
        link.put(gl)
        out["first"] = conv_backward(first, g1)
        assert pair.take() is g1

    in_backward(body)
    assert out["first"] == (None, {"add": gl, "add2": None, "gate": False})
    assert not tag.masked


def test_sole_consumer_gate_needs_tag_declaration_and_eligibility():
    x, tag = relu_output()
    g = rnd(8)
    for links, gate_ok, want in ((Links(sole_consumer=True), True, True),
                                 (Links(sole_consumer=True), False, False),
                                 (Links(), True, False)):
        tag.masked = False
        got, asked = conv_backward(bound(links, x), g, gate_ok)
        assert got is g and asked["gate"] is want and tag.masked is want
    got, asked = conv_backward(bound(Links(sole_consumer=True)), g)  # an untagged input
    assert not asked["gate"]


# --------------------------------------------------------- top-down Pair
def topdown_pair(lateral_is_mfma=True):
    td, merged = Pair(topdown=True), torch.zeros(1, requires_grad=True)
    out_conv = bound(Links(pair=td))
    assert td.output_is_mfma
    H.tag(merged, H.TD_PAIR, td)
    lateral = bound(Links(), topdown=merged) if lateral_is_mfma else None
    return td, out_conv, lateral


def test_topdown_pair_without_an_mfma_lateral_is_ignored():
    td, out_conv, _ = topdown_pair(lateral_is_mfma=False)
    g = rnd(9)
    assert conv_backward(out_conv, g) == (g, {"add": None, "add2": None, "gate": False})
    assert td.empty


def test_topdown_pair_needs_a_registered_output_conv_and_a_differentiable_map():
    merged = torch.zeros(1, requires_grad=True)
    H.tag(merged, H.TD_PAIR, Pair(topdown=True))  # (its output conv was no MFMA conv)
    assert bound(Links(), topdown=merged).td_pair is None
    td, frozen = Pair(topdown=True), torch.zeros(1)
    bound(Links(pair=td))
    H.tag(frozen, H.TD_PAIR, td)
    assert bound(Links(), topdown=frozen).td_pair is None and not td.lateral_is_mfma


@pytest.mark.parametrize("lateral_first", [False, True])
def test_topdown_pair_both_orders(lateral_first):
    td, out_conv, lateral = topdown_pair()
    assert lateral.td_pair is td and td.lateral_is_mfma
    gtd, gout = rnd(10), rnd(11)
    out = {}

    def body():
        if lateral_first:
            out["lat"] = td.meet_topdown(gtd)
            out["conv"] = conv_backward(out_conv, gout)
        else:
            out["conv"] = conv_backward(out_conv, gout)
            out["lat"] = td.meet_topdown(gtd)

    in_backward(body)
    if lateral_first:
        assert out["lat"] is None
        got, asked = out["conv"]
        assert got is gout and asked["add"] is gtd
    else:
        assert out["conv"] == (None, {"add": None, "add2": None, "gate": False})
        assert torch.equal(out["lat"], gtd + gout)
    assert td.empty


# ------------------------------------------- DeferredPixels through a Pair
def test_deferred_pixels_run_into_an_ungated_dgrad_without_add():
    pair, pooled, g = Pair(), rnd(12), rnd(13)
    px = FakePixels(pooled)
    conv = bound(Links(pair=pair))
    want = g + pooled
    out = {}

    def body():
        pair.deposit(px, "RPN head / ROI pooler level")
        out["conv"] = conv_backward(conv, g)

    in_backward(body)
    got, asked = out["conv"]
    assert asked == {"add": None, "add2": None, "gate": False}
    assert got is g and torch.equal(got, want) and px.runs == ["add_into"]
    assert pair.empty


@pytest.mark.parametrize("why", ["gated", "adding"])
def test_deferred_pixels_are_materialized_for_a_gated_or_adding_dgrad(why):
    pair, link, pooled, g, gl = Pair(), Slot(), rnd(14), rnd(15), rnd(16)
    px = FakePixels(pooled)
    x, tag = relu_output()
    if why == "gated":
        conv = bound(Links(sole_consumer=True, pair=pair), x)
    else:
        conv = bound(Links(grad_from=link, pair=pair))
    out = {}

    def body():
        if why == "adding":
            link.put(gl)
        pair.deposit(px, "RPN head / ROI pooler level")
        out["conv"] = conv_backward(conv, g)

    in_backward(body)
    got, asked = out["conv"]
    assert got is g and px.runs == ["materialize"]
    assert asked["gate"] is (why == "gated") and tag.masked is (why == "gated")
    assert torch.equal(asked["add"], pooled if why == "gated" else gl + pooled)


def test_deferred_pixels_refuse_a_wrong_map():
    px = FakePixels(rnd(17))
    for bad in (torch.zeros(2, 4, 5, 4), torch.zeros(SHAPE, dtype=torch.float64),
                torch.zeros(2, 4, 8, 5).transpose(2, 3)):
        with pytest.raises(ValueError):
            px.add_into(bad)
    assert px.runs == []


# ------------------------------------------------------------------- join
def join_members(tagged_producer=True):
    x, tag = relu_output() if tagged_producer else (torch.zeros(1), None)
    pair = Pair()
    m1, m2 = bound(Links(pair=pair), x), bound(Links(pair=pair), x)
    lat = bound(Links(join=pair), x)
    pair.join_lateral()
    return pair, tag, m1, m2, lat


@pytest.mark.parametrize("tagged_producer", [True, False])
def test_join_lateral_last(tagged_producer):
    pair, tag, m1, m2, lat = join_members(tagged_producer)
    d1, d2, dl = rnd(20), rnd(21), rnd(22)
    out = {}

    def body():
        out[1] = conv_backward(m1, d1)
        assert pair.g is d1 and pair.sum is None and pair.lat is None
        out[2] = conv_backward(m2, d2)
        assert pair.g is None and pair.sum is d2 and pair.lat is None
        assert pair.completed_by is None
        out[3] = conv_backward(lat, dl)

    in_backward(body)
    assert out[1] == (None, {"add": None, "add2": None, "gate": False})
    assert out[2][0] is None and out[2][1]["add"] is d1 and not out[2][1]["gate"]
    got, asked = out[3]
    assert got is dl and asked["add"] is d2 and asked["add2"] is None
    assert asked["gate"] is tagged_producer
    assert tag is None or tag.masked
    assert pair.completed_by == "lateral" and pair.empty


@pytest.mark.parametrize("lateral_first", [False, True])
@pytest.mark.parametrize("tagged_producer", [True, False])
def test_join_pair_last(lateral_first, tagged_producer):
    pair, tag, m1, m2, lat = join_members(tagged_producer)
    d1, d2, dl = rnd(23), rnd(24), rnd(25)
    out = {}

    def body():
        if lateral_first:
            out["lat"] = conv_backward(lat, dl)
            out[1] = conv_backward(m1, d1)
        else:
            out[1] = conv_backward(m1, d1)
            out["lat"] = conv_backward(lat, dl)
        assert pair.g is d1 and pair.lat is dl and pair.sum is None
        assert pair.completed_by is None and (tag is None or not tag.masked)
        out[2] = conv_backward(m2, d2)

    in_backward(body)
    for k in (1, "lat"):
        assert out[k] == (None, {"add": None, "add2": None, "gate": False})
    got, asked = out[2]
    assert got is d2 and asked["add"] is d1 and asked["add2"] is dl  # (dgrad + g) + lat
    assert asked["gate"] is tagged_producer
    assert tag is None or tag.masked
    assert pair.completed_by == "pair" and pair.empty


def test_join_gate_eligibility_binds_the_lateral_only():
    # the lateral gates in its dgrad epilogue (needs an eligible conv); the pair
    # member's (dgrad + add) + add2 pass gates for any conv
    for last in ("lateral", "pair"):
        pair, tag, m1, m2, lat = join_members()
        out = {}

        def body():
            order = (m1, m2, lat) if last == "lateral" else (lat, m1, m2)
            for m in order:
                out[last] = conv_backward(m, rnd(26), gate_ok=False)

        in_backward(body)
        assert out[last][1]["gate"] is (last == "pair") and tag.masked is (last == "pair")
        assert pair.completed_by == last


def test_join_pair_member_materializes_deferred_pixels():
    pair, tag, m1, m2, lat = join_members()
    pooled = rnd(27)
    px = FakePixels(pooled)
    out = {}

    def body():
        pair.deposit(px, "RPN head / ROI pooler level")
        out[2] = conv_backward(m2, rnd(28))

    in_backward(body, lambda: conv_backward(lat, rnd(28)))
    assert pair.empty and px.runs == ["materialize"] and torch.equal(out[2][1]["add"], pooled)


def test_join_is_off_for_a_conv_with_a_residual_link():
    pair, link = Pair(), Slot()
    pair.join_lateral()
    conv = bound(Links(grad_from=link, pair=pair))
    gl, g = rnd(29), rnd(30)
    out = {}

    def body():
        link.put(gl)
        out["conv"] = conv_backward(conv, g)  # the plain pair protocol: first deposits
        assert pair.take() is g

    in_backward(body)
    assert out["conv"] == (None, {"add": gl, "add2": None, "gate": False})


# -------------------------------------------------------- LevelAccumulator
def test_level_accumulator_sums_in_arrival_order_and_starts_over():
    acc = LevelAccumulator(3)
    gs = [rnd(31), rnd(32), rnd(33)]
    want = (gs[0] + gs[1]) + gs[2]
    assert not torch.equal(want, gs[0] + (gs[1] + gs[2]))  # (the order matters on these)
    for _ in range(2):
        got = []
        in_backward(lambda: got.extend(
            acc.accumulate(lambda old, g=g: g.clone() if old is None else old.add_(g))
            for g in gs))
        assert got[0] is None and got[1] is None and torch.equal(got[2], want)
        assert acc.empty


def test_level_accumulator_hands_deferred_items_over_in_arrival_order():
    acc = LevelAccumulator(3)
    items = [(rnd(34), rnd(35)), (rnd(36), rnd(37)), (rnd(38), rnd(39))]
    for _ in range(2):
        got = []
        in_backward(lambda: got.extend(acc.defer(it) for it in items))
        assert got[0] is None and got[1] is None
        assert len(got[2]) == 3 and all(a is b for a, b in zip(got[2], items))
        assert acc.empty


# ------------------------------------------------------------- PoolerShare
def test_pooler_share_assigns_set0_and_set1_by_arrival():
    share = PoolerShare()
    box, mask = ("boxes0", "ind0", rnd(40), "p0"), ("boxes1", "ind1", rnd(41), "p1")
    out = []

    def backward(mine):  # the merged branch of ops.roi._RoIAlignFn.backward
        first = share.rois.take()
        if first is None:
            share.rois.put(mine)
            return None
        return first, mine

    in_backward(lambda: out.append(backward(mask)), lambda: out.append(backward(box)))
    assert out[0] is None and out[1] == (mask, box) and share.empty


def test_pooler_share_hands_the_maps_over_unmerged():
    share = PoolerShare()
    maps = [rnd(42), rnd(43)]
    out = []

    def backward():
        prior = share.maps.take()
        if prior is None:
            share.maps.put(maps)
        out.append(prior)

    in_backward(backward, backward)
    assert out[0] is None and out[1] is maps and share.empty


# ------------------------------------------------------- incomplete passes
def raises_then_recovers(first_only, both, empty):
    """A pass that reaches only the first participant raises and leaves the
    object empty; a complete pass afterwards succeeds."""
    with pytest.raises(HandoffError):
        in_backward(first_only)
    assert empty()
    x = in_backward(*both)
    assert x.grad is not None and empty()


def test_incomplete_slot_raises_and_clears():
    link = Slot()
    raises_then_recovers(lambda: link.put(rnd(50)),
                         (lambda: link.put(rnd(50)), link.take), lambda: link.empty)


def test_incomplete_pair_raises_and_clears():
    pair = Pair()
    a, b = bound(Links(pair=pair)), bound(Links(pair=pair))
    raises_then_recovers(lambda: conv_backward(a, rnd(51)),
                         (lambda: conv_backward(a, rnd(51)), lambda: conv_backward(b, rnd(52))),
                         lambda: pair.empty)


def test_incomplete_topdown_pair_raises_and_clears():
    td, out_conv, _ = topdown_pair()
    raises_then_recovers(lambda: td.meet_topdown(rnd(53)),
                         (lambda: td.meet_topdown(rnd(53)),
                          lambda: conv_backward(out_conv, rnd(54))), lambda: td.empty)


@pytest.mark.parametrize("reached", [("m1",), ("lat",), ("m1", "m2"), ("m1", "lat")])
def test_incomplete_join_raises_and_clears(reached):
    pair, tag, m1, m2, lat = join_members()
    members = {"m1": m1, "m2": m2, "lat": lat}
    step = lambda m: (lambda: conv_backward(m, rnd(55)))  # noqa: E731
    with pytest.raises(HandoffError):
        in_backward(*(step(members[k]) for k in reached))
    assert pair.empty and not tag.masked
    in_backward(step(m1), step(lat), step(m2))
    assert pair.empty and tag.masked and pair.completed_by == "pair"


@pytest.mark.parametrize("deferred", [False, True])
def test_incomplete_level_accumulator_raises_and_clears(deferred):
    acc = LevelAccumulator(3, "RPN head 1x1 weight-gradient levels")
    if deferred:
        arrive = lambda: acc.defer((rnd(56), rnd(57)))  # noqa: E731
    else:
        arrive = lambda: acc.accumulate(lambda old: rnd(56) if old is None else old + 1)  # noqa: E731
    with pytest.raises(HandoffError, match="RPN head 1x1 weight-gradient levels"):
        in_backward(arrive, arrive)
    assert acc.empty
    out = []
    in_backward(*[lambda: out.append(arrive())] * 3)
    assert out[0] is None and out[1] is None and out[2] is not None and acc.empty


def test_incomplete_pooler_share_raises_and_clears():
    share = PoolerShare()
    raises_then_recovers(lambda: share.rois.put("set 0"),
                         (lambda: share.maps.put("maps"), share.maps.take),
                         lambda: share.empty)


def test_handoff_error_names_the_protocol():
    with pytest.raises(HandoffError, match="gradient hand-off 'residual' was not completed"):
        in_backward(lambda: Slot().put(rnd(58)))


# ---------------------------------------------------------------- observer
def test_observer_sees_every_protocol_by_its_label(monkeypatch):
    assert H.OBSERVER is None  # unset by default: one `is None` test per event
    seen = []
    monkeypatch.setattr(H, "OBSERVER", lambda label, event: seen.append((label, event)))
    link, pair, share = Slot(), Pair(), PoolerShare()
    td, out_conv, _ = topdown_pair()
    jp, _, m1, m2, lat = join_members()
    jp2, _, n1, n2, lat2 = join_members()
    level = Pair()
    acc = LevelAccumulator(2, "shared conv weight-gradient calls")
    a, b = bound(Links(pair=pair)), bound(Links(pair=pair))
    px = FakePixels(rnd(60))

    def body():
        link.put(rnd(61))
        link.take()
        conv_backward(a, rnd(62))
        conv_backward(b, rnd(63))
        td.meet_topdown(rnd(64))
        conv_backward(out_conv, rnd(65))
        for m in (m1, m2, lat, lat2, n1, n2):
            conv_backward(m, rnd(66))
        share.rois.put("set 0")
        share.rois.take()
        level.deposit(px, "RPN head / ROI pooler level")
        conv_backward(bound(Links(pair=level)), rnd(67))
        acc.accumulate(lambda old: 1)
        acc.accumulate(lambda old: 2)

    in_backward(body)
    deposits = [label for label, event in seen if event == "deposit"]
    assert deposits == ["residual", "pair", "FPN top-down", "join (pair)", "join (sum)",
                        "join (lateral)", "join (pair)", "box/mask poolers",
                        "RPN head / ROI pooler level", "shared conv weight-gradient calls"]
    assert [s for s in seen if s[1] == "complete"] == [
        ("join (lateral)", "complete"), ("join (pair)", "complete"),
        ("shared conv weight-gradient calls", "complete")]
    assert ("deferred pixels", "apply level 2") in seen
    assert sum(1 for _, event in seen if event == "take") == 9
