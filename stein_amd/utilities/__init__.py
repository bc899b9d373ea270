from .compute_median import compute_median
from .converters import convert_array_to_dictionary, convert_dictionary_to_array
from .stein_discrepancy import kernelized_stein_discrepancy

__all__ = ["compute_median", "convert_array_to_dictionary", "convert_dictionary_to_array", "kernelized_stein_discrepancy"]
