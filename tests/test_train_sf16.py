"""The split-f16 conv-arithmetic mode of the CostRegNet training convolutions (train_ops.conv_arithmetic): the public interface,
without a GPU."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_arithmetic_values_and_restore():
    from cds_mvsnet_amd import train_ops
    before = train_ops.get_conv_arithmetic()
    for kind in ("f32", "split_f16"):
        with train_ops.conv_arithmetic(kind):
            assert train_ops.get_conv_arithmetic() == kind
        assert train_ops.get_conv_arithmetic() == before
    for bad in ("bf16", "fp16", "", None, "F32"):
        with pytest.raises(ValueError):
            train_ops.conv_arithmetic(bad)
        with pytest.raises(ValueError):
            train_ops.set_conv_arithmetic(bad)
    train_ops.set_conv_arithmetic("split_f16")
    try:
        assert train_ops.get_conv_arithmetic() == "split_f16"
    finally:
        train_ops.set_conv_arithmetic(before)


@pytest.mark.parametrize("env,want", [(None, "f32"), ("split_f16", "split_f16"), ("f32", "f32")])
def test_process_default_comes_from_environment(env, want):
    e = {k: v for k, v in os.environ.items() if k != "CDS_TRAIN_CONV"}
    if env is not None:
        e["CDS_TRAIN_CONV"] = env
    code = "import sys; sys.path.insert(0, %r); from cds_mvsnet_amd import train_ops; print(train_ops.get_conv_arithmetic())" % ROOT
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split()
    assert out[-1] == want


def test_train_step_and_captured_step_take_the_keyword():
    from cds_mvsnet_amd import train
    for fn in (train.train_step, train.CapturedTrainStep.__init__):
        p = inspect.signature(fn).parameters["conv_arithmetic"]
        assert p.default is None
    with pytest.raises(ValueError):
        train.CapturedTrainStep(None, None, conv_arithmetic="half")


def test_capture_key_holds_the_mode():
    """The capture key of CapturedTrainStep carries the resolved mode: a change of the mode (keyword or process default) is a new
    graph."""
    from cds_mvsnet_amd import train, train_ops
    st = train.CapturedTrainStep.__new__(train.CapturedTrainStep)
    st.conv_arithmetic = None
    with train_ops.conv_arithmetic("split_f16"):
        assert st._conv_mode() == "split_f16"
    with train_ops.conv_arithmetic("f32"):
        assert st._conv_mode() == "f32"
    st.conv_arithmetic = "split_f16"
    with train_ops.conv_arithmetic("f32"):
        assert st._conv_mode() == "split_f16"


def test_split_f16_keeps_the_stage_streams_off(monkeypatch):
    """CDS_TRAIN_STAGE_STREAMS=1 overlaps the stages' backward chains (ATen kernels included); the split-f16 mode's f16 MFMAs must not
    run next to ATen kernels (packed-fp32 hazard), so the mode keeps one stream."""
    from cds_mvsnet_amd import train_ops, training
    monkeypatch.setattr(training, "STAGE_STREAMS", True)
    monkeypatch.setattr(training, "BATCH_FEATURES", True)
    with train_ops.conv_arithmetic("f32"):
        assert training.stage_streams_enabled()
    with train_ops.conv_arithmetic("split_f16"):
        assert not training.stage_streams_enabled()
    monkeypatch.setattr(training, "STAGE_STREAMS", False)
    with train_ops.conv_arithmetic("f32"):
        assert not training.stage_streams_enabled()


def test_bad_environment_value_warns_and_keeps_f32():
    """CDS_TRAIN_CONV takes exactly the values conv_arithmetic() takes; anything else (including another letter case) leaves the
    default f32 with a warning instead of making the package unimportable."""
    e = dict(os.environ, CDS_TRAIN_CONV="F32")
    code = ("import sys, warnings; sys.path.insert(0, %r); warnings.simplefilter('always')\n"
            "with warnings.catch_warnings(record=True) as w:\n"
            "    from cds_mvsnet_amd import train_ops\n"
            "print(train_ops.get_conv_arithmetic(), any('CDS_TRAIN_CONV' in str(x.message) for x in w))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split()
    assert out[-2:] == ["f32", "True"]
