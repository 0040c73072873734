"""Registration of the drop-in plugin classes with the reference's orchestrator."""
_PKG = __name__.rsplit(".", 1)[0]
_ENSEMBLER = "audio_separator.separator.ensembler"
_ORCHESTRATOR = "audio_separator.separator.separator"


def install(architectures=("mdx", "mdxc", "demucs", "vr"), ensembler=False):
    """Make the reference's orchestrator load this package's plugin classes: ``Separator.load_model`` resolves its
    architecture class with ``importlib.import_module("audio_separator.separator.architectures.<arch>_separator")``
    (separator.py:903-904), so registering these modules under those names is the whole integration -- no line of the
    reference changes.  Call before ``Separator.load_model``; returns the list of names registered.

    ``ensembler=True`` also registers this package's ``Ensembler`` (ensemble.py) under ``audio_separator.separator.ensembler``
    -- and on ``audio_separator.separator.separator``, which binds the name at import (separator.py:26), when that module is
    already imported -- so that the orchestrator's ensemble combine runs on the device.  ``uninstall`` undoes both."""
    import importlib
    import sys
    done = []
    for a in architectures:
        mod = importlib.import_module(f"{_PKG}.architectures.{a}_separator")
        name = f"audio_separator.separator.architectures.{a}_separator"
        sys.modules[name] = mod
        parent = sys.modules.get("audio_separator.separator.architectures")
        if parent is not None:
            setattr(parent, f"{a}_separator", mod)
        done.append(name)
    if ensembler:
        mod = importlib.import_module(f"{_PKG}.ensemble")
        sys.modules[_ENSEMBLER] = mod
        parent = sys.modules.get("audio_separator.separator")
        if parent is not None:
            setattr(parent, "ensembler", mod)
        orch = sys.modules.get(_ORCHESTRATOR)
        if orch is not None:
            if not hasattr(mod, "_replaced_ensembler"):
                mod._replaced_ensembler = getattr(orch, "Ensembler", None)
            orch.Ensembler = mod.Ensembler
        done.append(_ENSEMBLER)
    return done


def uninstall():
    import sys
    for a in ("mdx", "mdxc", "demucs", "vr"):
        name = f"audio_separator.separator.architectures.{a}_separator"
        mod = sys.modules.get(name)
        if mod is not None and getattr(mod, "__name__", "").startswith(_PKG + "."):
            del sys.modules[name]
    mod = sys.modules.get(_ENSEMBLER)
    if mod is not None and getattr(mod, "__name__", "").startswith(_PKG + "."):
        del sys.modules[_ENSEMBLER]
        orch = sys.modules.get(_ORCHESTRATOR)
        if orch is not None and getattr(orch, "Ensembler", None) is mod.Ensembler:
            previous = mod.__dict__.pop("_replaced_ensembler", None)
            if previous is not None:
                orch.Ensembler = previous
            else:
                del orch.Ensembler

