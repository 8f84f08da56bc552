from .Propagation import Propagation  # noqa: F401
from .SimilarityFunctions import SimilarityFunctions  # noqa: F401
from .TaskDecoder import TaskDecoder  # noqa: F401
from .ToyGraphBase import ToyGraphBase  # noqa: F401
from .utility import (fewshot_mean_logits, fewshot_predict_labels_by_mean, fewshot_predict_logits,  # noqa: F401
                      process_tu_dataset, seed_everything)
