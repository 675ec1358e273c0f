import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle.binding import Oracle

    return Oracle()


@pytest.fixture(scope="session")
def ref():
    """The reference's answers: those recorded from its own object code in tests/golden/ref_answers.npz, everywhere.  Where
    oracle/_ref is built (or can be) every call also runs that object code and fails if it no longer gives the recorded answer."""
    from oracle.binding import RecordedRef, Ref, ref_available

    if not ref_available():
        return RecordedRef()
    return RecordedRef(live=Ref(), mode="check")


@pytest.fixture()
def ctx():
    """A FRESH device context through the C-ABI for every test (statistics hint, tier steering and XCD balance start from
    scratch: which kernel variant a test reaches does not depend on what ran before it).  Fails loudly if the HIP library
    is missing."""
    import hdr2yuv_amd as h

    c = h.Context(0)
    yield c
    c.close()
