"""The table of training switches (tests/train_switch_cases.py) against the sources it restates: it classifies exactly the non-EXPERIMENTS
rows of sola_amd/csrc/tune.h, so a key added later must be classified - training step or not, with its settings and its promise - before the
suite passes; and every promise of bit-identity quotes docs/tune_keys.md."""
import os
import re

import train_switch_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tune_h_keys():
    return T.parse_tune_keys(open(os.path.join(ROOT, "sola_amd", "csrc", "tune.h")).read())


def _flat(s):
    return re.sub(r"\s+", " ", s)


def test_the_table_classifies_exactly_the_keys_of_tune_h():
    keys = _tune_h_keys()
    assert len(keys) == len(set(keys)) and len(keys) >= 58
    assert not set(T.TRAINING) & set(T.NOT_TRAINING), set(T.TRAINING) & set(T.NOT_TRAINING)
    assert set(T.TRAINING) | set(T.NOT_TRAINING) == set(keys), set(keys) ^ (set(T.TRAINING) | set(T.NOT_TRAINING))


def test_the_parser_reads_tune_h_as_the_library_does():
    """the rows the parser finds are the keys the built library enumerates (sola_tune_key), in order; an EXPERIMENTS build enumerates its
    second list behind them"""
    from sola_amd import _lib
    built = []
    while _lib.lib().sola_tune_key(len(built)) is not None:
        built.append(_lib.lib().sola_tune_key(len(built)).decode())
    keys = _tune_h_keys()
    assert built[:len(keys)] == keys
    assert (len(built) > len(keys)) == _lib.has_experiments()


def test_every_entry_is_well_formed():
    for k, e in T.TRAINING.items():
        assert e["values"] and e["modes"] and set(e["modes"]) <= set(T.MODES), k
        p = e["promise"]
        for m in e["modes"]:
            assert T.promise(k, m) in ("bits", "order", "rounding"), (k, m)
        if isinstance(p, dict):
            assert set(p) == set(e["modes"]), k
        assert e["note"], k
        for v in e["values"]:
            x = T.bf16_expect(k, v)
            assert set(x) <= {"qkv16", "o16", "prenorm16"} and set(x.values()) <= {"all", "none", "motion", "o2l"}, (k, v)
        assert not e["bf16"] or "bf16" in e["modes"], k
        assert set(e["under"]) <= set(T.TRAINING) - {k}, k
    for k, why in T.NOT_TRAINING.items():
        assert re.match(r"[a-z_0-9]+\.hip", why), k  # names the file that reads it
    assert set(T.ACROSS) <= set(T.TRAINING)
    for (ka, _), (kb, _) in T.PAIRS:
        assert "bf16" in T.TRAINING[ka]["modes"] and "bf16" in T.TRAINING[kb]["modes"], (ka, kb)
    ids = [f"{m}-{k}-{v}" for m, k, v in T.settings()]
    assert len(ids) == len(set(ids))


def test_every_promise_of_bit_identity_quotes_the_catalogue():
    doc = open(os.path.join(ROOT, "docs", "tune_keys.md")).read()
    entries = [_flat(e) for e in re.split(r"^\* ", doc, flags=re.M)[1:]]
    for k, e in T.TRAINING.items():
        bits = [m for m in e["modes"] if T.promise(k, m) == "bits"]
        if not bits:
            assert e["cite"] is None, k
            continue
        assert e["cite"] and "bit-identical" in e["cite"], k
        hit = [x for x in entries if f'"{k}"' in x and _flat(e["cite"]) in x]
        assert hit, (k, e["cite"])


def test_default_values_are_not_listed_as_settings():
    from sola_amd import _lib
    for k, e in T.TRAINING.items():
        assert _lib.tune_default(k) not in e["values"], k
