"""``model.Exp1.Exp1`` — the class the reference resolves by name under MODEL_NAME=Exp1
(src/train.py:18: getattr(importlib.import_module(f"model.{model_name}"), model_name))."""
from newsrecommendationsystem_amd.exp1 import Exp1  # noqa: F401
