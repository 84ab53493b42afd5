"""The one statement of CostRegNet's wiring (model.costreg_unet) driven by a recording stand-in: which layer reads what, with which
stride and skip, when every intermediate is released, and where the slab halo hook is called.  No GPU, no library."""
import gc
import weakref

import torch

from cds_mvsnet_amd.model import costreg_unet


class Recorder:
    """Layers that compute nothing: fresh CPU tensors of the right relative shapes.  Logs (step, layer, stride, id of the input, id
    of the skip) and, on entry to every step, which of the tensors it handed out can still be reached."""

    def __init__(self, vol):
        self.log, self.readers, self.alive, self.refs, self.names = [], [], {}, {}, {id(vol): "vol"}

    def reachable(self):
        gc.collect()
        return {n for n, r in self.refs.items() if r() is not None}

    def _enter(self, step, name, stride, x, skip):
        self.alive[name] = self.reachable()
        self.log.append((step, name, stride, id(x), None if skip is None else id(skip)))
        # the same record with the ids resolved to the layers that produced the tensors
        self.readers.append((step, name, stride, self.names[id(x)], None if skip is None else self.names[id(skip)]))

    def _out(self, name, shape):
        t = torch.zeros(shape)
        self.refs[name] = weakref.ref(t)
        self.names[id(t)] = name          # an id is only looked up while its tensor is alive, so a reused id names the newer one
        return t

    def conv(self, name, x, stride):
        self._enter("conv", name, stride, x, None)
        return self._out(name, [d // stride for d in x.shape])

    def deconv(self, name, x, skip):
        self._enter("deconv", name, 2, x, skip)
        assert [2 * d for d in x.shape] == list(skip.shape), (name, x.shape, skip.shape)
        return self._out(name, skip.shape)

    def tail(self, x, skip, refresh):
        self._enter("tail", "conv11", 2, x, skip)
        assert [2 * d for d in x.shape] == list(skip.shape)
        y = self._out("conv11", skip.shape)
        refresh(y, 0, True, True)         # the slab layers' halo rows between conv11 and prob
        return self._out("prob", skip.shape)


def _run(refresh=None):
    vol = torch.zeros(16, 24, 40)         # three sizes, so a swapped axis shows in the shape checks
    rec = Recorder(vol)
    out = costreg_unet(rec, vol, refresh)
    return rec, out


def test_sequence_strides_and_skips():
    rec, out = _run()
    assert rec.readers == [("conv", "conv0", 1, "vol", None), ("conv", "conv1", 2, "conv0", None), ("conv", "conv2", 1, "conv1", None),
                       ("conv", "conv3", 2, "conv2", None), ("conv", "conv4", 1, "conv3", None), ("conv", "conv5", 2, "conv4", None),
                       ("conv", "conv6", 1, "conv5", None), ("deconv", "conv7", 2, "conv6", "conv4"),
                       ("deconv", "conv9", 2, "conv7", "conv2"), ("tail", "conv11", 2, "conv9", "conv0")]
    assert len(rec.log) == 10 and all(len(r) == 5 for r in rec.log)
    assert out is rec.refs["prob"]() and tuple(out.shape) == (16, 24, 40)


def test_intermediates_are_released_after_their_last_reader():
    """c1, c3, c5 go once the next layer consumed them, c4 after conv7, c2 after conv9, c0 after the tail; conv6's output and those of
    conv7 / conv9 go with the rebinding of the running value.  What a step finds alive is exactly what it or a later step reads."""
    rec, out = _run()
    rec.alive["returned"] = rec.reachable()
    assert rec.alive == {
        "conv0": set(),
        "conv1": {"conv0"},
        "conv2": {"conv0", "conv1"},
        "conv3": {"conv0", "conv2"},
        "conv4": {"conv0", "conv2", "conv3"},
        "conv5": {"conv0", "conv2", "conv4"},
        "conv6": {"conv0", "conv2", "conv4", "conv5"},
        "conv7": {"conv0", "conv2", "conv4", "conv6"},
        "conv9": {"conv0", "conv2", "conv7"},
        "conv11": {"conv0", "conv9"},
        "returned": {"prob"},
    }


def test_refresh_hook_follows_every_layer_read_across_a_slab_border():
    """The ten halo refreshes of slab_cost_regularization: a stride-2 layer reads one row above, a stride-1 layer one on each side, a
    transposed layer one coarse row below; the last one (between conv11 and prob) is made by the tail with the hook it was handed."""
    calls = []
    vol = torch.zeros(16, 24, 40)
    rec = Recorder(vol)
    costreg_unet(rec, vol, lambda y, level, need_top, need_bot: calls.append((rec.names[id(y)], level, need_top, need_bot, tuple(y.shape))))
    want = [("conv0", 0, True, False), ("conv1", 1, True, True), ("conv2", 1, True, False), ("conv3", 2, True, True),
            ("conv4", 2, True, False), ("conv5", 3, True, True), ("conv6", 3, False, True), ("conv7", 2, False, True),
            ("conv9", 1, False, True), ("conv11", 0, True, True)]
    assert [c[:4] for c in calls] == want
    assert all(c[4] == (16 >> c[1], 24 >> c[1], 40 >> c[1]) for c in calls)       # the level is that of the buffer handed over
