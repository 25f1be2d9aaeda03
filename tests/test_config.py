"""ginlite config engine tests (UX parity with gin-config usage in the
reference: utils.py:85-117, config/*.gin)."""

import os
import textwrap

import pytest

from genrec_amd.config import ginlite


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(textwrap.dedent(text))
    return str(p)


def test_macros_and_bindings(tmp_path):
    cfg = _write(tmp_path, "a.gin", """
        d_model = 128
        train.lr = 1e-3
        train.dims = [512, 256]
        train.name = "hello"
        train.d = %d_model
        train.flag = True
        train.none_val = None
    """)
    ginlite.parse_file(cfg)

    @ginlite.configurable(name="train")
    def train(lr=0.0, dims=None, name="", d=0, flag=False, none_val=1):
        return lr, dims, name, d, flag, none_val

    assert train() == (1e-3, [512, 256], "hello", 128, True, None)


def test_explicit_args_beat_bindings(tmp_path):
    cfg = _write(tmp_path, "b.gin", "f.x = 5\n")
    ginlite.parse_file(cfg)

    @ginlite.configurable(name="f")
    def f(x=0, y=0):
        return x, y

    assert f() == (5, 0)
    assert f(x=7) == (7, 0)


def test_split_substitution(tmp_path):
    cfg = _write(tmp_path, "c.gin", 'g.path = "out/{split}/ckpt"\n')
    ginlite.parse_file(cfg, substitutions={"split": "beauty"})

    @ginlite.configurable(name="g")
    def g(path=""):
        return path

    assert g() == "out/beauty/ckpt"


def test_class_reference(tmp_path):
    cfg = _write(tmp_path, "d.gin", "h.dataset = @MyDs\n")

    @ginlite.configurable(name="MyDs")
    class MyDs:
        def __init__(self, v=3):
            self.v = v

    ginlite.parse_file(cfg)

    @ginlite.configurable(name="h")
    def h(dataset=None):
        return dataset

    assert h() is MyDs


def test_enum_constant(tmp_path):
    cfg = _write(
        tmp_path, "e.gin",
        "q.mode = %genrec_amd.models.rqvae.QuantizeForwardMode.STE\n")
    ginlite.parse_file(cfg)
    from genrec_amd.models.rqvae import QuantizeForwardMode

    @ginlite.configurable(name="q")
    def q(mode=None):
        return mode

    assert q() is QuantizeForwardMode.STE


def test_include(tmp_path):
    _write(tmp_path, "base.gin", "base_val = 10\n")
    cfg = _write(tmp_path, "main.gin", """
        include "base.gin"
        z.v = %base_val
    """)
    ginlite.parse_file(cfg)

    @ginlite.configurable(name="z")
    def z(v=0):
        return v

    assert z() == 10


def test_cli_parse_config(tmp_path):
    cfg = _write(tmp_path, "f.gin", 'w.a = 1\nw.p = "x/{split}"\n')
    ginlite.parse_config([cfg, "--split", "toys", "--gin", "w.a=2"])

    @ginlite.configurable(name="w")
    def w(a=0, p=""):
        return a, p

    assert w() == (2, "x/toys")


def test_class_binding_injection():
    ginlite.bind("Klass.size", "9")

    @ginlite.configurable(name="Klass")
    class Klass:
        def __init__(self, size=1):
            self.size = size

    assert Klass().size == 9
    assert Klass(size=2).size == 2


def test_shipped_configs_parse():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel in ["config/sasrec/synthetic.gin", "config/hstu/synthetic.gin",
                "config/tiger/synthetic/tiger.gin",
                "config/tiger/synthetic/rqvae.gin"]:
        ginlite.clear_config()
        ginlite.parse_file(os.path.join(root, rel),
                           substitutions={"split": "beauty"})


def test_all_shipped_gin_configs_parse():
    """Every config/ gin file parses with {split} substitution: imports
    resolve, macros defined, enum constants resolvable."""
    import glob
    import os

    from genrec_amd.config import ginlite

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "config", "**", "*.gin"),
                             recursive=True))
    assert len(files) >= 12
    for f in files:
        ginlite.clear_config()
        ginlite.parse_file(f, substitutions={"split": "beauty"})
        if os.path.basename(f) != "base.gin":
            assert ginlite.get_bindings("train"), f


def test_call_reference_and_nested_refs(tmp_path):
    """@name() call-refs resolve at injection time; refs nested in lists."""
    from genrec_amd.config import ginlite

    ginlite.clear_config()

    @ginlite.configurable(name="make_thing")
    def make_thing(val: int = 3):
        return {"val": val}

    @ginlite.configurable(name="consumer")
    def consumer(thing=None, factories=None):
        return thing, factories

    cfg = tmp_path / "c.gin"
    cfg.write_text(
        "make_thing.val = 9\n"
        "consumer.thing = @make_thing()\n"
        "consumer.factories = [@make_thing, @consumer]\n")
    ginlite.parse_file(str(cfg))
    thing, factories = consumer()
    assert thing == {"val": 9}  # called at injection, bindings applied
    assert callable(factories[0]) and callable(factories[1])


def test_utils_decorators_and_debug_metrics():
    import torch

    from genrec_amd.modules.utils import compute_debug_metrics, eval_mode
    from genrec_amd.modules.utils import reset_kv_cache as reset_kv_deco

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 2)
            self.kv_cache = {"k": 1}
            self.was_training = None

        def reset_kv_cache(self):
            self.kv_cache = {}

        @eval_mode
        def infer(self):
            self.was_training = self.training
            return 1

        @reset_kv_deco
        def gen(self):
            return dict(self.kv_cache)

    m = M()
    m.train()
    assert m.infer() == 1
    assert m.was_training is False and m.training is True  # restored
    assert m.gen() == {}  # cache cleared before the call

    mask = torch.tensor([[1, 1, 0], [1, 1, 1]])
    d = compute_debug_metrics(mask)
    assert any("seq_length" in k for k in d)


def test_reference_gin_binding_names_are_drop_in():
    """Every `train.X` binding in the REFERENCE's shipped configs must be
    a parameter of the corresponding trainer here (config drop-in). The
    binding names of each reference config are stored, in file order, in
    tests/golden/reference_train_bindings.json."""
    import inspect
    import json

    from genrec_amd.trainers import (hstu_trainer, lcrec_trainer,
                                     rqvae_trainer, sasrec_trainer,
                                     tiger_trainer)

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "golden", "reference_train_bindings.json")
    with open(golden) as fh:
        bindings = json.load(fh)
    cases = {
        sasrec_trainer: ["sasrec/amazon.gin"],
        hstu_trainer: ["hstu/amazon.gin"],
        rqvae_trainer: ["tiger/amazon/rqvae.gin",
                        "lcrec/amazon/rqvae.gin"],
        tiger_trainer: ["tiger/amazon/tiger.gin"],
        lcrec_trainer: ["lcrec/amazon/lcrec.gin",
                        "lcrec/amazon/lcrec_debug.gin"],
    }
    assert sorted(f for fs in cases.values() for f in fs) == sorted(bindings)
    for mod, files in cases.items():
        params = set(inspect.signature(mod.train.__wrapped__).parameters)
        for f in files:
            assert bindings[f], f
            for name in bindings[f]:
                assert name in params, \
                    f"{mod.__name__} missing param {name} ({f})"


def test_circular_include_raises(tmp_path):
    from genrec_amd.config import ginlite

    a = tmp_path / "a.gin"
    b = tmp_path / "b.gin"
    a.write_text(f'include "{b}"\n')
    b.write_text(f'include "{a}"\n')
    import pytest

    with pytest.raises(ginlite.GinError, match="circular"):
        ginlite.parse_file(str(a))


def test_config_run_comments_reference_real_trainers():
    """Every `python -m genrec_amd.trainers.X` mentioned in config files
    and docs refers to an importable module."""
    import glob
    import importlib
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mods = set()
    for pattern in ("config/**/*.gin", "docs/*.md", "README.md"):
        for f in glob.glob(os.path.join(root, pattern), recursive=True):
            for m in re.finditer(r"genrec_amd\.trainers\.(\w+)", open(f).read()):
                mods.add(m.group(1))
    assert mods  # sanity: the docs do reference trainers
    for name in sorted(mods):
        importlib.import_module(f"genrec_amd.trainers.{name}")


def test_mkdocs_nav_files_exist():
    import yaml

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "mkdocs.yml")))
    for entry in cfg["nav"]:
        for _, path in entry.items():
            assert os.path.exists(os.path.join(root, path)), path


def test_unquoted_string_value_error_hints_quoting():
    import pytest

    from genrec_amd.config import ginlite

    with pytest.raises(ginlite.GinError, match="need quotes"):
        ginlite.bind("train.save_dir_root", "/tmp/nope")
