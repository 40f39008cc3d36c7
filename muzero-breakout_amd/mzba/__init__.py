"""mzba: MuZero on Breakout for the MI355X. The opt-in classes are reachable from the package by name and
imported on first use, so `import mzba` itself stays free of torch and of the HIP library."""
_OPT_IN = {"SinkArchive": "archive", "StagedWindows": "archive", "EpisodeStats": "stats", "Trainer": "train"}


def __getattr__(name):
    if name in _OPT_IN:
        import importlib
        return getattr(importlib.import_module(f".{_OPT_IN[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
