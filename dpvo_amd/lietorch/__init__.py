"""lietorch on MI355X: SO3 / SE3 / Sim3 groups over the `lietorch_backends` HIP
extension (L-SE3).

API of dpvo/lietorch (cuteboyqq/DPVO: groups.py, group_ops.py,
broadcasting.py): `SE3(data)`, `.inv()`, `*` (group product or action on
points), `.retr(a)`, `.adjT(a)`, `.matrix()`, `.log()`, `SE3.exp(a)`, ...
Sim3 (group id 4) is the group of the loop-closure pose graph
(dpvo_amd/loop_closure.py); its Exp / Log gradients and Jinv use the exact
left Jacobian, a deliberate deviation from the reference's truncated series.
RxSO3 (group id 2) is not provided by this build; constructing one raises.
"""
from .groups import LieGroup, LieGroupParameter, RxSO3, SE3, SO3, Sim3, cat, stack  # noqa: F401

__all__ = ["LieGroup", "LieGroupParameter", "SO3", "SE3", "RxSO3", "Sim3", "cat", "stack"]
