"""Host-side mirror of reference src/ddsp/utils.py."""
import torch


def modifed_sigmoid(x):
    """reference src/ddsp/utils.py:6-9 (spelling kept)."""
    return 2 * (torch.sigmoid(x) ** 2.3) + 1e-6
