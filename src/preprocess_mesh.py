# coding: utf-8
"""`src.preprocess_mesh` of the reference, served by diffudf_amd.preprocess_mesh (see src/__init__.py)."""
from diffudf_amd.preprocess_mesh import *  # noqa: F401,F403
from diffudf_amd import preprocess_mesh as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
