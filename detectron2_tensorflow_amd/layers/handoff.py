"""Gradient hand-offs between the autograd nodes of the fused training graph.

Several backwards hand a gradient to another backward instead of returning it,
so that the receiver adds it inside its own kernel epilogue: no autograd add of
two full maps, no separate ReLU-backward pass, no zero-fill of pooled levels.
This module holds the state machines of those hand-offs (torch only: it runs
on a CPU-only machine); the kernels are launched by their callers
(layers/conv_grad.py:_ConvMFMAFn, layers/ops/roi.py:_RoIAlignFn,
modeling/proposal_generator/rpn.py:_RPNHead1x1Fn).

``ReluTag`` -- fused-ReLU chains.  A conv with a fused ReLU tags its output.  A
consumer conv whose caller declares it the SOLE consumer of that output (the
bottleneck's conv2 / conv3, the mask head's chain and deconv, the RPN head's
fused 1x1) applies the producer's ReLU mask in its own dgrad epilogue and sets
``masked``; the producer then skips its threshold_backward.  Without the
declaration nothing is fused.

``Slot`` -- one value, put once and taken once, producer before consumer.  The
bottleneck's identity shortcut: the conv that adds ``residual`` gets the slot
as ``res_grad_to``, the conv that reads the same tensor as ``grad_from``.  The
adder's backward (always first: the reader's waits for the chain in between)
puts the residual's gradient there instead of returning it; the reader adds it
before the ReLU gate, so gx = (dgrad + g_res) * (x > 0) is one pass.

``Pair`` -- two readers of one tensor, either order.  The first backward
deposits its input gradient (ungated, nothing added) and returns none; the
second takes the deposit, adds it in its dgrad epilogue / stride scatter and
returns the sum.  Three uses:
  * the bottleneck's conv1 / projection shortcut (``pair_grad``);
  * ``Pair(topdown=True)``: an FPN merged map read by its output conv
    (``pair_grad``) and by the next finer lateral's fused top-down add, which
    finds the pair on the map (TD_PAIR tag).  Both must be MFMA convs: each
    registers in its forward, and the output conv ignores a pair no lateral
    registered with.  The lateral's side is ``meet_topdown``;
  * an FPN level read by the RPN head conv and the ROI poolers (LEVEL_PAIR
    tag).  The poolers' deposit may be a ``DeferredPixels``: the conv runs that
    pixel pass into its own full dgrad map afterwards when it neither gates
    nor adds, and takes the materialized map otherwise.

Join -- a Pair a third reader has joined (``join_lateral``): a ResNet stage
output x (a ReLU output) read by the next stage's conv1 / shortcut pair and by
the FPN lateral, which finds the pair on x (STAGE_PAIR tag) and gets it as
``join``.  Autograd would form lat + (pair2 + pair1) and then the producer's
threshold_backward; here
  * the first pair member deposits its dgrad (``g``, as without a join);
  * the second pair member forms s = dgrad + g; if the lateral's gradient is
    already there it returns gate((s) + lat) (one scatter pass for a strided
    1x1), else it deposits s (``sum``);
  * the lateral returns gate(dgrad + s) if s is there, else it deposits its own
    dgrad (``lat``).
The last one applies the producer's ReLU mask in the same pass and sets its
tag (``completed_by`` says which it was), so the sum and the gate are
bit-identical to the autograd formulation.  A conv with a residual link
(``grad_from``) never takes part in a join.

``Links`` carries one conv call's ends of the above into _ConvMFMAFn;
``Links.plan`` turns what has arrived into a ``Plan``: the operands of the ONE
dgrad call the backward makes, and what happens to its result.

``LevelAccumulator(n)`` -- a weight used by n calls of one forward (the RPN
head's convs over the FPN levels).  Every call's backward adds its weight
gradient to the running value (old + new, in backward-arrival order: autograd's
order for the summed gradients) or defers its (input, gradient) pair; every
arrival but the n-th gets nothing, the n-th the result, and the accumulator
starts over (a second backward of the same graph).

``RowBound`` -- a bound on the non-zero rows of a gradient that only its
producer can know (the RPN loss: the sampled anchors), declared by that
producer and handed down to the backwards that can skip the zero rows (the
RPN head's shared 3x3: a row census per level, made where the gradient is
still 16 wide, then a weight gradient over the non-zero 32-pixel chunks and a
data gradient over the rows whose 3x3 window holds a non-zero row).
Undeclared means dense everywhere.

``PoolerShare`` -- the box and mask poolers of a training step, which pool the
SAME maps.  Merged backward: the first arrival leaves its (boxes, box_ind,
grad_out, params) as set 0 and the second runs one backward over both sets.
Unmerged: the first writes the full maps and leaves them, the second
accumulates into them.

``WgradJoin`` -- the weight gradients of the convs whose weight is a batched
FrozenBN fold's output (the trainable backbone).  Nothing reads such a gradient
before the fold's own backward, which runs once, after every conv's: each conv
deposits its (input, output gradient, geometry) and returns no weight
gradient, and the fold's backward computes all of them in one grouped launch
per kernel family (ops.conv2d_wgrad_group): three launches and three reduces
off the chain of data gradients instead of 36 + 36 inside it, with the bits of
the single launches (tuning "wgrad_group" = 1; 2 also shortens the splits).

Every protocol assumes that all its participants' backwards run in the same
backward pass.  A backward that reaches only some of them (torch.autograd.grad
or .backward on a subset of the losses, a loss that detaches one branch) would
otherwise drop the deposited gradient silently: every deposit queues an engine
callback that runs when the backward pass ends and raises ``HandoffError`` if
the deposit is still there (clearing it first, so a later backward starts
clean).

``OBSERVER``: when set, called with (label, event) on every "deposit", "take"
and "complete", and with ("deferred pixels", "apply level <l>") when a deferred
pixel pass runs into a map (tests count hand-offs with it).
"""
import torch

_ENGINE = torch.autograd.Variable._execution_engine

OBSERVER = None


class HandoffError(RuntimeError):
    pass


def _msg(what):
    return (f"gradient hand-off '{what}' was not completed in this backward pass: the "
            "fused training graph needs every loss that reaches the shared features in ONE "
            "backward (sum the losses, or build the model with the hand-offs disabled)")


def _deposit(obj, field, value, label):
    """obj.field = value, checked at the end of the current backward pass (the
    first failing check ends the pass: it clears the whole object)."""
    setattr(obj, field, value)

    def check():
        if getattr(obj, field) is not None:
            obj.clear()
            raise HandoffError(_msg(label))

    _ENGINE.queue_callback(check)
    if OBSERVER is not None:
        OBSERVER(label, "deposit")


def _take(obj, field, label):
    value = getattr(obj, field)
    if value is not None:
        setattr(obj, field, None)
        if OBSERVER is not None:
            OBSERVER(label, "take")
    return value


# The tensor attributes the hand-off objects travel on, from the forward that
# makes them to the forward of the other participant.
RELU = "_d2mi_relu_info"         # a fused-ReLU conv output -> its ReluTag
STAGE_PAIR = "_d2mi_pair"        # a bottleneck input -> its conv1 / shortcut Pair
TD_PAIR = "_d2mi_td_pair"        # an FPN merged map -> its output conv's Pair
LEVEL_PAIR = "_d2mi_grad_pair"   # an FPN level -> its RPN conv / ROI pooler Pair
ROW_BOUND = "_d2mi_row_bound"    # the RPN head's concatenated logits -> its RowBound
FOLD_ENTRY = "_d2mi_fold_entry"  # a batched fold's w_eff -> (its WgradJoin, entry index)


def tag(t, name, value):
    setattr(t, name, value)


def tagged(t, name):
    return getattr(t, name, None)


class ReluTag:
    __slots__ = ("masked",)

    def __init__(self):
        self.masked = False


class Slot:
    __slots__ = ("value", "label")

    def __init__(self, label="residual"):
        self.value = None
        self.label = label

    @property
    def empty(self):
        return self.value is None

    def clear(self):
        self.value = None

    def put(self, value):
        _deposit(self, "value", value, self.label)

    def take(self):
        return _take(self, "value", self.label)


class DeferredPixels:
    """The pixel pass of ONE level of a merged ROIAlign backward
    (d2mi_roi_align_bwd2_ex phase 2), deposited for the backward that writes
    that level's full gradient map.  add_into(gx) adds the pooled
    contributions into gx in place (old + new at each touched pixel: the
    rounding of autograd's sum of the two maps); materialize() returns the
    pooled map alone (a fresh zeroed map + the pass), for a consumer that
    cannot take it afterwards."""
    __slots__ = ("_run", "level", "shape", "device")

    def __init__(self, run, level, shape, device):
        self._run, self.level, self.shape, self.device = run, level, tuple(shape), device

    def add_into(self, gx):
        if (tuple(gx.shape) != self.shape or gx.dtype != torch.float32 or not gx.is_contiguous()
                or gx.device != self.device):
            raise ValueError(f"deferred ROIAlign pixels: need a contiguous f32 {self.shape} map")
        if OBSERVER is not None:
            OBSERVER("deferred pixels", f"apply level {self.level}")
        self._run(self.level, gx, True)
        return gx

    def materialize(self):
        m = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        self._run(self.level, m, False)
        return m


class Pair:
    __slots__ = ("g", "sum", "lat", "topdown", "output_is_mfma", "lateral_is_mfma", "joined",
                 "completed_by")

    def __init__(self, topdown=False):
        self.g = self.sum = self.lat = None
        self.topdown = topdown
        self.output_is_mfma = self.lateral_is_mfma = False
        self.joined = False
        self.completed_by = None  # "lateral" / "pair": the member that completed the join

    @property
    def empty(self):
        return self.g is None and self.sum is None and self.lat is None

    def clear(self):
        self.g = self.sum = self.lat = None

    def deposit(self, value, label="pair"):
        _deposit(self, "g", value, label)

    def take(self):
        return _take(self, "g", "pair")

    def meet_topdown(self, gtd):
        """The lateral's side of a top-down pair: None for the first of the
        two (gtd is deposited), gtd + the output conv's deposit for the second."""
        other = self.take()
        if other is None:
            self.deposit(gtd, "FPN top-down")
            return None
        return gtd + other

    def join_lateral(self):
        """A lateral reads the pair's tensor too: the pair members now leave
        their sum to it (Links.plan)."""
        self.joined = True

    def _deposit_first(self, gx):
        _deposit(self, "g", gx, "join (pair)")

    def _deposit_sum(self, gx):
        _deposit(self, "sum", gx, "join (sum)")

    def _deposit_lateral(self, gx):
        _deposit(self, "lat", gx, "join (lateral)")

    def _complete(self, member):
        self.completed_by = member
        if OBSERVER is not None:
            OBSERVER(f"join ({member})", "complete")


class Plan:
    """What a conv backward does with its input gradient: gx = dgrad (+ add)
    (+ add2), through the ReLU gate of its input when ``gate``; ``finish(gx)``
    then sets the producer's tag (mark_masked), runs a deferred pixel pass
    into gx and either hands gx on (deposit_to: returns None) or returns it."""
    __slots__ = ("add", "add2", "deferred", "deposit_to", "mark_masked")

    def __init__(self, add=None, add2=None, deferred=None, deposit_to=None, mark_masked=None):
        self.add, self.add2, self.deferred = add, add2, deferred
        self.deposit_to, self.mark_masked = deposit_to, mark_masked

    @property
    def gate(self):
        return self.mark_masked is not None

    def finish(self, gx):
        if self.mark_masked is not None:
            self.mark_masked.masked = True
        if self.deferred is not None:
            gx = self.deferred.add_into(gx.contiguous())
        if self.deposit_to is not None:
            self.deposit_to(gx)
            return None
        return gx


class Links:
    """One conv call's ends of the hand-offs (all optional)."""
    __slots__ = ("sole_consumer", "res_grad_to", "grad_from", "pair", "join", "wacc", "in_tag",
                 "producer_tag", "td_pair", "rows")

    def __init__(self, sole_consumer=False, res_grad_to=None, grad_from=None, pair=None,
                 join=None, wacc=None, rows=None):
        self.sole_consumer = sole_consumer
        self.res_grad_to, self.grad_from = res_grad_to, grad_from
        self.pair, self.join, self.wacc = pair, join, wacc
        self.rows = rows  # (RowBound, level) of the output gradient, or None
        self.in_tag = self.producer_tag = self.td_pair = None

    def bind(self, x, topdown, has_residual):
        """Forward: read the tags of this call's inputs, register with the
        top-down pairs."""
        # the producer's ReLU tag: gated on by the sole consumer, or by a join
        self.producer_tag = tagged(x, RELU)
        self.in_tag = self.producer_tag if self.sole_consumer else None
        if not has_residual:
            self.res_grad_to = None
        if self.pair is not None and self.pair.topdown:
            self.pair.output_is_mfma = True
        if topdown is not None:
            td = tagged(topdown, TD_PAIR)
            if td is not None and td.output_is_mfma and topdown.requires_grad:
                td.lateral_is_mfma = True
                self.td_pair = td

    def plan(self, gate_ok):
        """gate_ok: this conv's dgrad can apply a ReLU gate in its epilogue."""
        join = self.join if self.join is not None else self.pair
        if join is not None and join.joined and self.grad_from is None:
            return self._plan_join(gate_ok)
        add = self.grad_from.take() if self.grad_from is not None else None
        gate_tag = self.in_tag if gate_ok else None
        pair = self.pair
        if pair is None or (pair.topdown and not pair.lateral_is_mfma):
            # (no pair, or an FPN output conv whose map no MFMA lateral reads)
            return Plan(add, mark_masked=gate_tag)
        other = pair.take()
        deferred = None
        if isinstance(other, DeferredPixels):
            # the ROI poolers' pixel pass of this level, run into this dgrad's
            # full map afterwards (no add here); a gated or already-adding
            # dgrad takes the pooled map instead
            if add is None and gate_tag is None:
                deferred, other = other, None
            else:
                other = other.materialize()
        if other is None and deferred is None:
            return Plan(add, deposit_to=pair.deposit)  # first of the pair: no gate
        if other is not None:
            add = other if add is None else add + other
        return Plan(add, deferred=deferred, mark_masked=gate_tag)

    def _plan_join(self, gate_ok):
        if self.join is not None:  # the lateral
            p = self.join
            s = _take(p, "sum", "join (sum)")
            if s is None:
                return Plan(deposit_to=p._deposit_lateral)
            p._complete("lateral")
            return Plan(s, mark_masked=self.producer_tag if gate_ok else None)
        p = self.pair
        other = p.take()
        if isinstance(other, DeferredPixels):
            other = other.materialize()
        if other is None:
            return Plan(deposit_to=p._deposit_first)
        lat = _take(p, "lat", "join (lateral)")
        if lat is None:
            return Plan(other, deposit_to=p._deposit_sum)
        p._complete("pair")
        # ((dgrad + other) + lat, gated: the caller's scatter pass or its fallback)
        return Plan(other, lat, mark_masked=self.producer_tag)


class LevelAccumulator:
    __slots__ = ("n", "k", "buf", "deferred", "label")

    def __init__(self, n, label="shared weight-gradient calls"):
        self.n, self.k, self.label = n, 0, label
        self.buf = None
        self.deferred = []

    @property
    def empty(self):
        return self.k == 0 and self.buf is None and not self.deferred

    def clear(self):
        self.k, self.buf, self.deferred = 0, None, []

    def _check(self):
        if self.k != 0:
            self.clear()
            raise HandoffError(_msg(self.label))

    def _arrive(self):
        self.k += 1
        if self.k == 1:
            # every call's backward must run in this pass, else the gradient
            # never leaves and a stale buffer would poison a later backward
            _ENGINE.queue_callback(self._check)
        last = self.k == self.n
        if OBSERVER is not None:
            OBSERVER(self.label, "complete" if last else "deposit")
        return last

    def accumulate(self, step):
        """One arrival: buf = step(buf) (step adds this call's share to the
        running value, None at the first).  None, or at the n-th arrival buf."""
        last = self._arrive()
        self.buf = step(self.buf)
        if not last:
            return None
        out = self.buf
        self.clear()
        return out

    def defer(self, item):
        """One arrival that leaves ``item`` for the last: None, or at the
        n-th arrival the items in arrival order."""
        last = self._arrive()
        self.deferred.append(item)
        if not last:
            return None
        out = self.deferred
        self.clear()
        return out


class RowBound:
    """A declared bound on the non-zero pixel rows of a gradient, per image,
    carried from the loss that knows it to the backwards that can use it (the
    RPN head: the loss has a gradient on the sampled anchors only, the head's
    fused 1x1 maps a zero row to a zero row, and it is the sole consumer of
    the shared 3x3's output).  One object per head forward, ``n`` levels.

    Undeclared (``declare`` never called): every level is dense, as without
    the object.  Declared: the 1x1's backward at level l runs a row census
    where ``wants_census`` and ``publish``es it (None = dense) for level l;
    the 3x3's backward ``take``s it, once, after it was published, and hands
    it to its weight and data gradients.  ``dilate``: (k, leading pad) of that
    data gradient's window, by which the census dilates its row list.  Nothing is
    ever inferred from the gradient's values: a false declaration sets the
    device error word (the census counts against ``capacity``).

    ``sparse_launches`` counts the launches that used a census (tests)."""
    __slots__ = ("n", "dilate", "rows_per_image", "_published", "sparse_launches")

    _EMPTY = object()

    def __init__(self, n, dilate=None):
        self.n = n
        # (k, leading pad) of the stride-1 conv window the census row lists are
        # dilated by: the consumer's data gradient (None: no lists)
        self.dilate = dilate
        self.rows_per_image = None
        self._published = [RowBound._EMPTY] * n
        self.sparse_launches = 0

    @property
    def declared(self):
        return self.rows_per_image is not None

    def declare(self, rows_per_image):
        rows_per_image = int(rows_per_image)
        if rows_per_image <= 0:
            raise ValueError("RowBound: rows_per_image must be positive")
        self.rows_per_image = rows_per_image

    def capacity(self, N):
        """Most non-zero rows of a level's gradient over N images."""
        return N * self.rows_per_image if self.declared else None

    def list_capacity(self, N):
        """Most rows of a level's dilated list: k * k per non-zero row."""
        k = self.dilate[0] if self.dilate else 0
        return k * k * self.capacity(N) if self.declared else None

    def wants_census(self, N, M):
        """A level of M pixel rows over N images is worth a census: even with
        every non-zero row's 3x3 neighbourhood counted, most rows are zero."""
        return self.declared and 9 * N * self.rows_per_image < M

    # wants_list: the list's capacity (k * k rows per non-zero row) against the
    # level's rows.  Measured on the MI355X ("Sparse RPN-head
    # backward"): the row-list data gradient wins clearly at 1/29 of the rows
    # (p2), about breaks even at 1/7 (p3) and loses at 1/2 (p4), where the fill,
    # the list's two extra census launches and the under-filled grid cost more
    # than the dense launch.
    LIST_MAX_FRACTION = 1.0 / 16

    def wants_list(self, N, M):
        """The census of a level of M rows should carry the dilated row list."""
        return (self.dilate is not None and self.wants_census(N, M)
                and self.list_capacity(N) <= M * type(self).LIST_MAX_FRACTION)

    def publish(self, level, census):
        self._published[level] = census

    def take(self, level):
        census = self._published[level]
        if census is RowBound._EMPTY:
            raise HandoffError(f"row bound: level {level} was not published (or taken twice)")
        self._published[level] = RowBound._EMPTY
        return census


class WgradJoin:
    """The weight gradients of the convs that read one batched fold's outputs
    (layers/ops/fold.py:_FoldManyFn), deferred to that fold's backward: nothing
    reads a folded conv's weight gradient before it, and it runs once, after
    every such conv's backward.  A conv whose weight IS the fold's output
    (FOLD_ENTRY tag) deposits (entry, x, gy, stride, pads, want_bias) here and
    returns no weight / bias gradient; the fold's backward takes every deposit
    and computes them in one grouped launch per kernel family.  A backward
    that ends with deposits left (the fold's backward did not run in it)
    raises HandoffError and clears them."""
    __slots__ = ("items", "label")

    def __init__(self, label="deferred weight gradients"):
        self.items = None
        self.label = label

    @property
    def empty(self):
        return self.items is None

    def clear(self):
        self.items = None

    def deposit(self, item):
        if self.items is None:
            _deposit(self, "items", [item], self.label)
        else:
            self.items.append(item)
            if OBSERVER is not None:
                OBSERVER(self.label, "deposit")

    def take_all(self):
        return _take(self, "items", self.label) or []


class PoolerShare:
    __slots__ = ("rois", "maps")

    def __init__(self):
        self.rois = Slot("box/mask poolers")  # merged backward: the first arrival's ROI set
        self.maps = Slot("box/mask poolers")  # unmerged: the first arrival's full maps

    @property
    def empty(self):
        return self.rois.empty and self.maps.empty
