"""Plugin interface of CLIPScore models: a ScoreModel whose score is the cosine of an image and a text embedding."""
from abc import abstractmethod
from typing import List

import torch

from ..model import ScoreModel


class CLIPScoreModel(ScoreModel):
    @abstractmethod
    def forward(self, images: List[str], texts: List[str]) -> torch.Tensor:
        """One cosine per (image, text) pair, pairs given as two parallel lists."""
