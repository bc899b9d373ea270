from .compute_median import compute_median
from .converters import convert_array_to_dictionary, convert_dictionary_to_array
from .stein_discrepancy import kernelized_stein_discrepancy
from .stein_test import ksd_quadratic_forms, stein_goodness_of_fit
from .stein_thinning import stein_thinning
from .stein_weights import stein_importance_weights, stein_kernel_products

__all__ = ["compute_median", "convert_array_to_dictionary", "convert_dictionary_to_array", "kernelized_stein_discrepancy",
           "ksd_quadratic_forms", "stein_goodness_of_fit", "stein_importance_weights", "stein_kernel_products", "stein_thinning"]
