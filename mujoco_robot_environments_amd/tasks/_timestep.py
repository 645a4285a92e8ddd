"""What ``reset()`` and ``step()`` of every task env return: dm_env's ``TimeStep`` / ``StepType`` and its array spec where
dm_env is installed (it is what the reference returns), an equivalent tuple, enum and spec where it is not."""
import collections
import enum

import numpy as np

try:
    import dm_env
    from dm_env import specs as _specs
    TimeStep, StepType = dm_env.TimeStep, dm_env.StepType
    _Array = _specs.Array
except Exception:  # pragma: no cover - dm_env absent on the target image
    class StepType(enum.IntEnum):
        FIRST = 0
        MID = 1
        LAST = 2

    TimeStep = collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])

    class _Array:
        def __init__(self, shape, dtype, name=None):
            self.shape, self.dtype, self.name = tuple(shape), np.dtype(dtype), name

        def __repr__(self):
            return f"Array(shape={self.shape}, dtype={self.dtype}, name={self.name})"
