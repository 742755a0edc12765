"""Host-side schedules for the update bits (NitiModel.set_update_bits): in NITI the number of bits
kept of the weight gradient is the learning rate, and the paper lowers it over the epochs."""
from __future__ import annotations


def bits_schedule(epoch: int, start: int, milestones) -> int:
    """The paper's staircase: `start` bits, one fewer from each milestone epoch on, never below 1:
    start - (number of milestones <= epoch), floored at 1."""
    return max(1, int(start) - sum(1 for m in milestones if int(m) <= int(epoch)))
