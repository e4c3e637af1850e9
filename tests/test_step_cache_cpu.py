"""The step cache's host side: the C ABI's two new names, argument checks that run before any launch, the hit / miss rule of
alg_amd.step_cache.StepCache on hand-made sums, the pass keys of the pipelines, run.py's flag.  No GPU."""
import argparse
import ctypes
import os
import re

import pytest

import alg_amd
from alg_amd.step_cache import StepCache, pass_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alg_step_cache_probe", "alg_step_cache_workspace_bytes")
INF, NAN = float("inf"), float("nan")


def test_header_exports_and_library_agree_on_the_two_names():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    lib = alg_amd.load_library()
    for name in NAMES:
        assert name in declared and name in alg_amd._lib.EXPORTS and hasattr(lib, name), name
    assert callable(alg_amd._lib.step_cache_probe) and callable(alg_amd._lib.step_cache_workspace_bytes)
    assert lib.alg_version() == 110


def test_workspace_query_is_a_host_function():
    lib = alg_amd.load_library()
    n = lib.alg_step_cache_workspace_bytes(229, 512)
    assert n > 0 and n % 16 == 0
    assert alg_amd._lib.step_cache_workspace_bytes(229, 512) == n
    big = lib.alg_step_cache_workspace_bytes(75600, 5120)          # Wan C5: the grid is capped, so is the workspace
    assert big % 16 == 0 and n < big <= 2048 * 16
    assert lib.alg_step_cache_workspace_bytes(0, 512) >= 16       # rows == 0 is fine
    assert lib.alg_step_cache_workspace_bytes(229, 516) == -1
    assert b"alg_step_cache_workspace_bytes" in lib.alg_last_error()


def test_probe_argument_errors_come_before_any_launch():
    lib = alg_amd.load_library()
    bufs = [(ctypes.c_char * 4096)() for _ in range(5)]
    keep, x1, r, work, sums = (ctypes.c_void_p((ctypes.addressof(b) + 63) // 64 * 64) for b in bufs)

    def call(keep=keep, x1=x1, r=r, rows=4, D=64, tok0=1, tok_rows=3, work=work, sums=sums):
        rc = lib.alg_step_cache_probe(keep, x1, r, rows, D, tok0, tok_rows, work, sums, None)
        return rc, lib.alg_last_error()

    for null in ("keep", "x1", "r", "work", "sums"):
        rc, msg = call(**{null: None})
        assert rc == -1 and b"alg_step_cache_probe" in msg and b"null" in msg, null
    rc, msg = call(D=516)
    assert rc == -1 and b"alg_step_cache_probe" in msg and b"multiple of 8" in msg
    for off in ("keep", "x1", "r"):
        rc, msg = call(**{off: ctypes.c_void_p(locals()[off].value + 2)})
        assert rc == -1 and b"alg_step_cache_probe" in msg and b"aligned" in msg, off
    for tok0, tok_rows in ((2, 3), (0, 5), (-1, 2), (1, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
        rc, msg = call(tok0=tok0, tok_rows=tok_rows)
        assert rc == -1 and b"alg_step_cache_probe" in msg and b"token rows" in msg, (tok0, tok_rows)
    rc, msg = call(x1=keep)
    assert rc == -1 and b"distinct" in msg
    rc, msg = call(rows=-1, tok0=0, tok_rows=0)
    assert rc == -1 and b"alg_step_cache_probe" in msg


# ---- the rule ------------------------------------------------------------------------------------------------------------
def forward(sc, sums, keys, force=False):
    """What a transformer does around `decide`: a computed forward ends with fresh tails for its keys."""
    hit = sc.decide(sums, keys, force)
    if not hit:
        sc.mark_valid(keys)
    return hit


def test_first_forward_misses_then_the_threshold_rules():
    sc = StepCache(threshold=0.5)
    k = ["uncond", "cond"]
    assert forward(sc, [(0.0, 1.0), (0.0, 1.0)], k) is False              # nothing cached yet, however small the change
    assert forward(sc, [(0.4, 1.0), (0.99, 2.0)], k) is True               # a < tau * b for every key
    assert forward(sc, [(0.5, 1.0), (0.1, 2.0)], k) is False               # a == tau * b is not a hit
    assert forward(sc, {"uncond": (0.1, 1.0), "cond": (0.1, 1.0)}, k) is True      # a mapping works too
    assert [r["hit"] for r in sc.stats] == [False, True, False, True]
    assert sc.stats[0]["rel"] == [INF, INF] and sc.stats[1]["rel"] == [0.4, 0.495] and sc.stats[1]["keys"] == k
    assert all(r["forced"] is False for r in sc.stats)


@pytest.mark.parametrize("bad", [(0.0, 0.0), (NAN, 1.0), (1.0, NAN), (INF, 1.0), (1.0, INF), (0.1, -1.0)])
def test_degenerate_sums_are_misses(bad):
    sc = StepCache(threshold=1e30)
    assert forward(sc, [(1.0, 1.0)], ["cond"]) is False
    assert forward(sc, [(1.0, 1.0)], ["cond"]) is True
    assert forward(sc, [bad], ["cond"]) is False
    assert forward(sc, [(1.0, 1.0)], ["cond"]) is True


def test_one_failing_key_of_three_makes_the_forward_a_miss():
    sc = StepCache(threshold=0.1)
    k = ["uncond_init", "uncond", "cond"]
    small = (0.01, 1.0)
    assert forward(sc, [small] * 3, k) is False
    assert forward(sc, [small] * 3, k) is True
    for i in range(3):
        sums = [small] * 3
        sums[i] = (0.2, 1.0)
        assert forward(sc, sums, k) is False, i
        assert forward(sc, [small] * 3, k) is True


def test_consecutive_hit_cap_force_reset_and_unseen_keys():
    sc = StepCache(threshold=1e30, max_consecutive=2)
    k, s = ["uncond", "cond"], [(1.0, 1.0), (1.0, 1.0)]
    assert [forward(sc, s, k) for _ in range(7)] == [False, True, True, False, True, True, False]
    sc.max_consecutive = 0                                                 # no cap
    assert [forward(sc, s, k) for _ in range(5)] == [True] * 5
    assert forward(sc, s, k, force=True) is False and sc.stats[-1]["forced"] is True
    assert forward(sc, s, k) is True
    # a key never seen makes the forward a miss, and is cached behind it: the 3-pass -> 2-pass hand-over in reverse
    k3, s3 = ["uncond_init"] + k, [(1.0, 1.0)] * 3
    assert forward(sc, s3, k3) is False
    assert forward(sc, s3, k3) is True
    assert forward(sc, s, k) is True                                       # "uncond" and "cond" carry over to the 2-pass steps
    sc.reset()
    assert sc.stats == []
    assert forward(sc, s, k) is False                                      # after a reset the next forward is computed
    assert forward(sc, s, k) is True
    # a computed forward that never finished (no mark_valid) leaves its keys unusable
    assert sc.decide(s, k, True) is False
    assert sc.decide(s, k) is False
    with pytest.raises(ValueError):
        sc.decide([(1.0, 1.0)], k)


def test_pass_keys_name_roles_not_rows():
    assert pass_keys(3, 1) == ["uncond_init", "uncond", "cond"]
    assert pass_keys(2, 1) == ["uncond", "cond"]
    assert pass_keys(1, 1) == ["cond"]
    assert pass_keys(2, 2) == [("uncond", 0), ("uncond", 1), ("cond", 0), ("cond", 1)]
    assert set(pass_keys(2, 1)) < set(pass_keys(3, 1))
    with pytest.raises(ValueError):
        pass_keys(4, 1)


def test_transformers_carry_the_switches_and_hunyuan_does_not():
    from alg_amd.step_cache import StepCacheHost, active
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    for cls in (CogVideoXTransformer3DModel, WanTransformer3DModel):
        assert issubclass(cls, StepCacheHost)
        assert isinstance(cls.step_cache, float) and cls.step_cache == 0.0
        assert isinstance(cls.step_cache_max_consecutive, int) and cls.step_cache_max_consecutive == 0
    assert not hasattr(HunyuanVideoTransformer3DModel, "step_cache")

    class StandIn:
        pass

    assert active(StandIn()) is False                                      # the loops' stand-in transformers are left alone
    host = StepCacheHost()
    assert active(host) is False and host.step_cache_stats == []
    host.step_cache = 0.1
    assert active(host) is True
    host.reset_step_cache()
    assert host.step_cache_stats == []


def test_run_py_flag_and_the_hunyuan_refusal():
    import run
    assert run.make_parser().parse_args([]).step_cache == 0.0
    args = run.make_parser().parse_args(["--step_cache", "0.1", "--config", os.path.join(ROOT, "configs", "hunyuan_video_alg.yaml")])
    assert args.step_cache == 0.1
    import yaml
    with open(args.config) as f:
        config = yaml.safe_load(f)
    assert "HunyuanVideo" in config["model"]["path"]
    with pytest.raises(SystemExit, match="--step_cache"):
        run.build_pipeline(config, args, "cpu")
    ns = argparse.Namespace(fp8=False, fp8_attention=False, synthetic=True, model_cache_dir=None, step_cache=-1.0)
    with pytest.raises(SystemExit, match="--step_cache"):
        run.build_pipeline({"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}, ns, "cpu")
