#!/usr/bin/env python3
"""Record the reference's answers to the calls tests/test_oracle.py makes of it (the `ref` fixture) into
tests/golden/ref_answers.npz, by running those tests with the reference's own object code (oracle/_ref)
behind a recording oracle.binding.RecordedRef.  Needs oracle/_ref (or the reference's sources to build it).

    python tests/golden/make_ref_answers.py

Run it again whenever one of those tests changes the inputs it passes to `ref`; elsewhere the tests answer
from the file alone, and where oracle/_ref exists they fail on any call the file does not hold."""
import importlib.util
import inspect
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import binding as ob  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("test_oracle", os.path.join(os.path.dirname(HERE), "test_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    oracle = ob.Oracle()
    rec = ob.RecordedRef(live=ob.Ref(), mode="record")
    for name, fn in sorted(vars(mod).items()):
        if name.startswith("test_") and callable(fn) and "ref" in inspect.signature(fn).parameters:
            fn(oracle, rec)
            print("recorded", name)
    rec.save()
    print(f"{len(rec.answers)} answers -> {os.path.relpath(rec.path)} ({os.path.getsize(rec.path)} bytes)")


if __name__ == "__main__":
    main()
