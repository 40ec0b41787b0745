"""MI355X-native NRMS news-recommendation scoring (drop-in for
Maguire1999/NewsRecommendationSystem's ``model.NRMS``).

    from newsrecommendationsystem_amd import NRMS, NRMSConfig
"""
from .config import BaseConfig, Exp1Config, NRMSConfig  # noqa: F401
from .nrms import NRMS  # noqa: F401
from .exp1 import Exp1  # noqa: F401
from .fit import ImpressionSet, TrainSet, fit  # noqa: F401

__all__ = ["NRMS", "NRMSConfig", "Exp1", "Exp1Config", "BaseConfig", "fit", "TrainSet", "ImpressionSet"]
