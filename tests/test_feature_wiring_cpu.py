"""The one statement of FeatureNet's wiring (model.feature_pyramid) driven by a recording stand-in: which layer reads what at which
pyramid level, the curvature triples, when every intermediate is released, and when the stages are handed out.  No GPU, no library."""
import gc
import weakref

import torch

from cds_mvsnet_amd.model import feature_pyramid

N, H, W = 5, 24, 40                        # three sizes, so a swapped axis shows in the shape checks


class Recorder:
    """Layers that compute nothing: fresh CPU tensors of the right relative shapes.  Logs (step, layer, level, producers of the inputs)
    and, on entry to every step, which of the activations it handed out can still be reached; `events` interleaves the steps with the
    emit calls."""

    def __init__(self, imgs):
        self.readers, self.events, self.alive, self.refs, self.names = [], [], {}, {}, {id(imgs): "imgs"}
        self.curvs, self.features = [], {}

    def reachable(self):
        gc.collect()
        return {n for n, r in self.refs.items() if r() is not None}

    def emit(self, name, stage):
        self.events.append(("emit", name, stage))

    def _enter(self, step, name, level, *inputs):
        self.alive[name] = self.reachable()
        self.readers.append((step, name, level, tuple(self.names[id(x)] for x in inputs)))
        self.events.append((step, name))

    def _named(self, name, shape):
        t = torch.zeros(shape)
        self.names[id(t)] = name          # an id is only looked up while its tensor is alive, so a reused id names the newer one
        return t

    def _act(self, name, shape):
        t = self._named(name, shape)
        self.refs[name] = weakref.ref(t)
        return t

    def dyn(self, name, x, level):
        self._enter("dyn", name, level, x)
        assert tuple(x.shape)[1:] == (H >> level, W >> level) and x.shape[0] in (3, N), (name, x.shape)      # imgs: 3 channels
        return self._act(name, (N, H >> level, W >> level)), self._named("nc " + name, (N, H >> level, W >> level))

    def down(self, name, x):
        self._enter("down", name, None, x)
        return self._act(name, (N, x.shape[1] // 2, x.shape[2] // 2))

    def lateral(self, name, coarse, skip):
        self._enter("lateral", name, None, coarse, skip)
        assert (N, 2 * coarse.shape[1], 2 * coarse.shape[2]) == tuple(skip.shape), (name, coarse.shape, skip.shape)
        return self._act(name, skip.shape)

    def head(self, name, x, level, stage):
        self._enter("head", name, level, x)
        assert tuple(x.shape) == (N, H >> level, W >> level) and stage == 3 - level, (name, x.shape, level, stage)
        self.features[stage] = (self._named(f"chw{stage}", x.shape), self._named(f"hwc{stage}", x.shape))
        return self.features[stage], self._act(name, x.shape) if stage == 2 else None, self._named("nc " + name, x.shape)

    def curv(self, a, b, c):
        assert a.shape == b.shape == c.shape
        self.curvs.append((tuple(self.names[id(t)] for t in (a, b, c)), (self._named("nc_sum", a.shape), self._named("nc_abs", a.shape))))
        return self.curvs[-1][1]


def _run(emit=True):
    imgs = torch.zeros(3, H, W)
    rec = Recorder(imgs)
    out = feature_pyramid(rec, imgs, rec.emit if emit else None)
    return rec, out


def test_sequence_levels_and_inputs():
    rec, _ = _run()
    assert rec.readers == [
        ("dyn", "conv00", 0, ("imgs",)), ("dyn", "conv01", 0, ("conv00",)), ("down", "downsample1", None, ("conv01",)),
        ("dyn", "conv10", 1, ("downsample1",)), ("dyn", "conv11", 1, ("conv10",)), ("down", "downsample2", None, ("conv11",)),
        ("dyn", "conv20", 2, ("downsample2",)), ("dyn", "conv21", 2, ("conv20",)),
        ("head", "out1", 2, ("conv21",)),
        ("lateral", "inner1", None, ("conv21", "conv11")), ("head", "out2", 1, ("inner1",)),
        ("lateral", "inner2", None, ("out2", "conv01")), ("head", "out3", 0, ("inner2",))]        # "out2": the stage-2 activation
    from cds_mvsnet_amd import FeatureNet
    assert sorted(r[1] for r in rec.readers) == sorted(name for name, _ in FeatureNet(8).named_children())       # every layer, once


def test_curvature_triples():
    rec, _ = _run()
    assert [names for names, _ in rec.curvs] == [("nc conv20", "nc conv21", "nc out1"), ("nc conv10", "nc conv11", "nc out2"),
                                                 ("nc conv00", "nc conv01", "nc out3")]


def test_intermediates_are_released_after_their_last_reader():
    """c00 goes after conv01, d0 and c10 after conv11, d1 and c20 after conv21, c21 and c11 after inner1, the stage-2 activation and c01
    after inner2; inner1's output goes when inner2's replaces it.  What a step finds alive is exactly what it or a later step reads
    (and, for inner2, the lateral output it is about to replace)."""
    rec, out = _run()
    rec.alive["returned"] = rec.reachable()
    assert rec.alive == {
        "conv00": set(),
        "conv01": {"conv00"},
        "downsample1": {"conv01"},
        "conv10": {"conv01", "downsample1"},
        "conv11": {"conv01", "downsample1", "conv10"},
        "downsample2": {"conv01", "conv11"},
        "conv20": {"conv01", "conv11", "downsample2"},
        "conv21": {"conv01", "conv11", "downsample2", "conv20"},
        "out1": {"conv01", "conv11", "conv21"},
        "inner1": {"conv01", "conv11", "conv21"},
        "out2": {"conv01", "inner1"},
        "inner2": {"conv01", "inner1", "out2"},
        "out3": {"inner2"},
        "returned": set(),
    }


def test_stages_are_emitted_before_the_next_lateral_is_launched():
    """Stage 1 is handed out before inner1 is launched and stage 2 before inner2 (what lets the coarse stages start on a side stream next
    to the finer FPN levels); stage 3 is only returned.  Without an emit the same steps run."""
    rec, out = _run()
    kinds = [e[:2] for e in rec.events]
    assert [e for e in kinds if e[0] == "emit"] == [("emit", "stage1"), ("emit", "stage2")]
    assert kinds.index(("head", "out1")) + 1 == kinds.index(("emit", "stage1")) == kinds.index(("lateral", "inner1")) - 1
    assert kinds.index(("head", "out2")) + 1 == kinds.index(("emit", "stage2")) == kinds.index(("lateral", "inner2")) - 1
    for e in rec.events:
        if e[0] == "emit":
            assert e[2] is out[e[1]]
    quiet, _ = _run(emit=False)
    assert quiet.events == [e for e in rec.events if e[0] != "emit"] and quiet.readers == rec.readers


def test_result_is_what_head_and_curv_returned():
    rec, out = _run()
    assert list(out) == ["stage1", "stage2", "stage3"]
    for k, stage in enumerate(("stage1", "stage2", "stage3")):
        want = rec.features[k + 1] + rec.curvs[k][1]
        assert len(out[stage]) == 4 and all(a is b for a, b in zip(out[stage], want))
        assert tuple(out[stage][0].shape) == (N, H >> (2 - k), W >> (2 - k))
