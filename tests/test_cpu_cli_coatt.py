"""test.py --coatt {bf16,mxfp8}: the option is parsed, defaults to bf16, and mxfp8 without
--feature-bank or with --dtype fp32 is an argparse error (exit code 2) raised by get_arguments,
before anything touches the GPU.  Each refusal is identified by its own message, so none of
these passes because --coatt is merely unknown."""
import pytest

import test as test_cli


def test_coatt_option_and_default():
    assert test_cli.get_arguments(["--feature-bank", "--coatt", "mxfp8"]).coatt == "mxfp8"
    assert test_cli.get_arguments([]).coatt == "bf16"
    assert test_cli.get_arguments(["--feature-bank"]).coatt == "bf16"
    # bf16 needs neither the bank nor the bf16 dtype
    assert test_cli.get_arguments(["--coatt", "bf16"]).coatt == "bf16"
    a = test_cli.get_arguments(["--feature-bank", "--coatt", "bf16", "--dtype", "fp32"])
    assert (a.coatt, a.dtype, a.feature_bank) == ("bf16", "fp32", True)


@pytest.mark.parametrize("argv,message", [
    (["--coatt", "mxfp8"], "--coatt mxfp8 needs --feature-bank"),
    (["--dtype", "bf16", "--coatt", "mxfp8"], "--coatt mxfp8 needs --feature-bank"),
    (["--feature-bank", "--dtype", "fp32", "--coatt", "mxfp8"], "--coatt mxfp8 needs --dtype bf16"),
    (["--feature-bank", "--coatt", "int4"], "argument --coatt: invalid choice: 'int4'"),
])
def test_coatt_mxfp8_needs_the_bf16_bank(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        test_cli.get_arguments(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
