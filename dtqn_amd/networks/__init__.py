"""Network factory surface: `DTQN` (dtqn/networks/dtqn.py:12-218) and the recurrent baseline `DRQN` (dtqn/networks/drqn.py:9-66),
resolved on first access."""

__all__ = ["DTQN", "DRQN"]


def __getattr__(name):
    if name == "DTQN":
        from .dtqn import DTQN
        return DTQN
    if name == "DRQN":
        from .drqn import DRQN
        return DRQN
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
