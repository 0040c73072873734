#!/usr/bin/env python3
"""Tables read from the REFERENCE package for the CPU tests (build container only), stored as tests/golden/reference_tables.json:

  stem_constants       every upper-case class constant of the reference's CommonSeparator (stem names, STEM_PAIR_MAPPER,
                       NON_ACCOM_STEMS, ...), as Python literals;
  roformer_normaliser  the reference ConfigurationNormalizer on each YAML of tests/test_host_files.py::YAMLS and each model path:
                       the normalised configuration (Python literal) and its detected model type, or the name of the error raised.

    python tests/golden/make_golden_reference_tables.py
"""
import ast
import importlib
import importlib.machinery
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
from tests.test_host_files import ROFORMER_PATHS, YAMLS  # noqa: E402


def stem_constants():
    tree = ast.parse(open(REF + "/audio_separator/separator/common_separator.py").read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "CommonSeparator")
    ns = {}
    for node in cls.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id.isupper():
            exec(compile(ast.Module([node], []), "ref_constants", "exec"), ns)
    return {k: repr(v) for k, v in sorted(ns.items()) if k.isupper()}


def roformer_normaliser():
    for n, path in (("audio_separator", REF + "/audio_separator"), ("audio_separator.separator", REF + "/audio_separator/separator")):
        pkg = types.ModuleType(n)
        pkg.__path__ = [path]
        pkg.__spec__ = importlib.machinery.ModuleSpec(n, None, is_package=True)
        sys.modules[n] = pkg
    ref = importlib.import_module("audio_separator.separator.roformer.configuration_normalizer").ConfigurationNormalizer()
    out = {}
    for name, cfg in sorted(YAMLS.items()):
        for path in ROFORMER_PATHS:
            try:
                want = ref.normalize_from_file_path(cfg, path, apply_defaults=True, validate=True)
            except Exception as e:
                out[f"{name}|{path}"] = {"error": type(e).__name__}
                continue
            assert ast.literal_eval(repr(want)) == want, (name, path)
            out[f"{name}|{path}"] = {"config": repr(want), "model_type": ref.detect_model_type(want)}
    return out


if __name__ == "__main__":
    tables = {"stem_constants": stem_constants(), "roformer_normaliser": roformer_normaliser()}
    with open(os.path.join(HERE, "reference_tables.json"), "w") as fh:
        json.dump(tables, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print({k: len(v) for k, v in tables.items()})
