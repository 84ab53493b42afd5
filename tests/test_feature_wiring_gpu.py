"""The launch sequence of FeatureNet on its three sets of layers (model.feature_pyramid driven by the channels-last runner, the planar
runner and training.feature_net): the names of the C entry points called, in order, against literal lists recorded before the three
written-out copies of the pyramid became one.  Batch of 4 images of 32x64 (n_shared = 2, n_chw = 2): the smallest extents at which
every level still has W % 4 == 0 (64, 32, 16) and the shared reference copies, the CHW / HWC split and the side hand-off all run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = [
    "cds_dynconv_cl_parts", "cds_conv00_cl_sf16_f32", "cds_instnorm_reduce_f32", "cds_dynconv_cl_parts",
    "cds_dynconv_cl_sf16_f32", "cds_instnorm_reduce_f32", "cds_conv2d_k3s2_cl_sf16_f32", "cds_instnorm_stats_cl_parts",
    "cds_instnorm_stats_cl_f32", "cds_instnorm_reduce_f32", "cds_dynconv_cl_parts", "cds_dynconv_cl_sf16_f32",
    "cds_instnorm_reduce_f32", "cds_dynconv_cl_parts", "cds_dynconv_cl_sf16_f32", "cds_instnorm_reduce_f32",
    "cds_conv2d_k3s2_cl_sf16_f32", "cds_instnorm_stats_cl_parts", "cds_instnorm_stats_cl_f32", "cds_instnorm_reduce_f32",
    "cds_dynconv_cl_parts", "cds_dynconv_cl_sf16_f32", "cds_instnorm_reduce_f32", "cds_dynconv_cl_parts",
    "cds_dynconv_cl_sf16_f32", "cds_instnorm_reduce_f32", "cds_dynconv_cl_parts", "cds_dynconv_cl_sf16_f32",
    "cds_instnorm_reduce_f32", "cds_instnorm_apply_cl_f32", "cds_curvature_stats_f32", "emit stage1",
    "cds_fpn_cl_parts", "cds_conv2d_fpn_cl_f32", "cds_instnorm_reduce_f32", "cds_dynconv_cl_parts",
    "cds_dynconv_cl_sf16_f32", "cds_instnorm_reduce_f32", "cds_instnorm_apply_cl_f32", "cds_curvature_stats_f32",
    "emit stage2", "cds_fpn_cl_parts", "cds_conv2d_fpn_cl_f32", "cds_instnorm_reduce_f32",
    "cds_dynconv_cl_parts", "cds_dynconv_cl_sf16_f32", "cds_instnorm_reduce_f32", "cds_instnorm_apply_cl_f32",
    "cds_curvature_stats_f32",
]
PLANAR = [
    "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_blend_stats_parts",
    "cds_dynconv_blend_stats_f32", "cds_instnorm_reduce_f32", "cds_dynconv_fused_parts", "cds_dynconv_fused_sbf_f32",
    "cds_instnorm_reduce_f32", "cds_conv2d_affine_f32", "cds_instnorm_affine_f32", "cds_dynconv_fused_parts",
    "cds_dynconv_fused_sbf_f32", "cds_instnorm_reduce_f32", "cds_dynconv_fused_parts", "cds_dynconv_fused_sbf_f32",
    "cds_instnorm_reduce_f32", "cds_conv2d_affine_f32", "cds_instnorm_affine_f32", "cds_dynconv_fused_parts",
    "cds_dynconv_fused_sbf_f32", "cds_instnorm_reduce_f32", "cds_dynconv_fused_parts", "cds_dynconv_fused_sbf_f32",
    "cds_instnorm_reduce_f32", "cds_dynconv_fused_parts", "cds_dynconv_fused_sbf_f32", "cds_instnorm_reduce_f32",
    "cds_instnorm_apply_f32", "cds_instnorm_apply_f32", "cds_curvature_stats_f32", "emit stage1",
    "cds_fpn_stats_parts", "cds_conv2d_fpn_f32", "cds_instnorm_reduce_f32", "cds_dynconv_fused_parts",
    "cds_dynconv_fused_sbf_f32", "cds_instnorm_reduce_f32", "cds_instnorm_apply_f32", "cds_chw_to_hwc_f32",
    "cds_chw_to_hwc_f32", "cds_curvature_stats_f32", "emit stage2", "cds_fpn_stats_parts",
    "cds_conv2d_fpn_f32", "cds_instnorm_reduce_f32", "cds_dynconv_fused_parts", "cds_dynconv_fused_sbf_f32",
    "cds_instnorm_reduce_f32", "cds_instnorm_apply_f32", "cds_instnorm_apply_f32", "cds_curvature_stats_f32",
]
TRAIN = [
    "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_conv2d_affine_f32",
    "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32",
    "cds_instnorm_act_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32",
    "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32",
    "cds_dynconv_blend_train_f32", "cds_instnorm_act_f32", "cds_pack_conv2d_f32", "cds_conv2d_affine_f32",
    "cds_instnorm_act_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_conv2d_affine_f32",
    "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32", "cds_instnorm_act_f32",
    "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_conv2d_affine_f32", "cds_conv2d_affine_f32",
    "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32", "cds_instnorm_act_f32", "cds_pack_conv2d_f32",
    "cds_conv2d_affine_f32", "cds_instnorm_act_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32",
    "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32",
    "cds_instnorm_act_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_conv2d_affine_f32",
    "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32", "cds_instnorm_act_f32",
    "cds_pack_conv2d_f32", "cds_pack_conv2d_f32", "cds_conv2d_affine_f32", "cds_conv2d_affine_f32",
    "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32", "cds_instnorm_act_f32", "cds_curvature_stats_f32",
    "cds_pack_conv2d_f32", "cds_conv2d_affine_f32", "cds_instnorm_act_f32", "cds_pack_conv2d_f32",
    "cds_pack_conv2d_f32", "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32",
    "cds_dynconv_blend_train_f32", "cds_instnorm_act_f32", "cds_curvature_stats_f32", "cds_pack_conv2d_f32",
    "cds_conv2d_affine_f32", "cds_instnorm_act_f32", "cds_pack_conv2d_f32", "cds_pack_conv2d_f32",
    "cds_conv2d_affine_f32", "cds_conv2d_affine_f32", "cds_dynconv_bn_stats_f32", "cds_dynconv_blend_train_f32",
    "cds_instnorm_act_f32", "cds_curvature_stats_f32",
]


class _Recording:
    """Stands in for the loaded library: logs the name of every entry point fetched from it (ops fetches one per call)."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        self._log.append(name)
        return getattr(self._lib, name)


@pytest.fixture()
def record(monkeypatch):
    from cds_mvsnet_amd import _lib
    log = []
    monkeypatch.setattr(_lib, "_lib", _Recording(_lib.load(), log))       # _lib.load() hands this out until the test ends
    return log


def test_launch_sequences(record, monkeypatch):
    import cds_mvsnet_amd.model as cm
    from cds_mvsnet_amd import FeatureNet, seeded_init_, training
    dev = torch.device("cuda:0")
    net = seeded_init_(FeatureNet(8), 7).to(dev).eval()
    g = torch.Generator().manual_seed(11)
    ref = torch.rand(3, 32, 64, generator=g)
    imgs = torch.stack([ref, ref] + [torch.rand(3, 32, 64, generator=g) for _ in range(2)]).to(dev)
    epi = torch.tensor([[20.0, -70.0], [90.0, 15.0], [-40.0, 50.0], [33.0, 120.0]])

    def infer():
        cm._FeatureRunner(net)(imgs, epi, 0.1, n_chw=2, n_shared=2, on_stage1=lambda name, stage: record.append("emit " + name))

    def recorded(run):
        run()                             # once unrecorded: weight packing and first-call caches
        del record[:]
        run()
        torch.cuda.synchronize()
        return list(record)

    with torch.no_grad():
        cl = recorded(infer)
        monkeypatch.setattr(cm, "USE_FEAT_CL", False)
        planar = recorded(infer)
    net.train()
    train = recorded(lambda: training.feature_net(net, imgs, epi.to(dev), 0.1, groups=2))
    for name, got in (("CL", cl), ("PLANAR", planar), ("TRAIN", train)):
        print(f"{name} = [")
        for i in range(0, len(got), 4):
            print("    " + " ".join(f'"{n}",' for n in got[i:i + 4]))
        print("]")
    assert cl == CL
    assert planar == PLANAR
    assert train == TRAIN
    # stage 1 is handed to the side stream before the first launch of inner1, stage 2 before that of inner2; stage 3 is returned
    # (a lateral's first entry point is the one that sizes its statistics records)
    for got, first in ((cl, "cds_fpn_cl_parts"), (planar, "cds_fpn_stats_parts")):
        inner1, inner2 = (i for i, n in enumerate(got) if n == first)
        assert [n for n in got if n.startswith("emit")] == ["emit stage1", "emit stage2"]
        assert got.index("emit stage1") < inner1 < got.index("emit stage2") < inner2
