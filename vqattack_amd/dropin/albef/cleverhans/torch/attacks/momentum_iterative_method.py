"""The reference ships this attack under tf2/attacks only; this is its module path under torch/attacks (albef copy)."""
import functools

from vqattack_amd import attacks as _impl

momentum_iterative_method = functools.wraps(_impl.momentum_iterative_method)(
    functools.partial(_impl.momentum_iterative_method, flavor="albef"))
