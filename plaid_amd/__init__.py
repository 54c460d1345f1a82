"""plaid_amd -- MI355X-native single-sample gene-set scoring behind the bigomics/plaid API.

Host side of the drop-in: the reference's R function names (`plaid`, `colranks`,
`normalize_medians`, `replaid.sing` ...) with dots as underscores, calling hand-written
gfx950 kernels through the C ABI of include/plaidhip.h.  See DESIGN.md / INTEGRATION.md.
"""
from ._lib import PlaidHipError, device_count
from .api import (aligned_pattern, chunked_crossprod, plaid_camera, plaid_camera_contrasts, plaid_fry, plaid_fry_contrasts, plaid_roast, plaid_roast_contrasts, plaid_romer, plaid_romer_contrasts, plaid_intergenecor, colranks, normalize_medians, plaid, plaid_fisher, plaid_gsea, plaid_limma, plaid_limma_contrasts, plaid_voom, plaid_rankcor, plaid_sig, plaid_test, plaid_test_contrasts, replaid_gsva,
                  replaid_gsva_exact, replaid_plage, replaid_zscore, replaid_aucell, replaid_scse, replaid_sing, replaid_sing_exact, replaid_ssgsea, replaid_ssgsea_exact, replaid_ucell,
                  replaid_ucell_exact, replaid_aucell_exact, sparse_colranks)
from .engine import (Context, Geneset, aucell_multi, camera_multi, fry_multi, roast_multi, romer_multi, default_context, fisher_multi, gsea_multi, gsea_multilevel_multi, limma_multi, voom_multi, gsva_exact_multi, gsva_kcdf_table, gsva_multi, multi_finalize, plaid_multi,
                     plaid_test_contrasts_multi, plaid_test_multi, plage_multi, zscore_multi, rankcor_multi, scse_multi, shard_bounds, sing_exact_multi, sing_multi, ssgsea_exact_multi, ssgsea_multi,
                     ucell_multi, ucell_exact_multi, aucell_exact_multi)
from .gmt import GmtList, gmt2mat, mat2gmt, read_gmt, write_gmt
from .matrix import NamedMatrix, as_named

__all__ = [
    "PlaidHipError", "device_count", "Context", "Geneset", "default_context", "NamedMatrix",
    "as_named", "GmtList", "read_gmt", "write_gmt", "gmt2mat", "mat2gmt", "plaid",
    "chunked_crossprod", "normalize_medians", "colranks", "sparse_colranks", "replaid_sing",
    "replaid_ssgsea", "replaid_ssgsea_exact", "replaid_ucell", "replaid_aucell", "replaid_scse", "aligned_pattern",
    "plaid_test", "replaid_gsva", "plaid_multi", "sing_multi", "ssgsea_multi", "ssgsea_exact_multi", "ucell_multi",
    "aucell_multi", "scse_multi", "gsva_multi", "replaid_gsva_exact", "gsva_exact_multi", "replaid_sing_exact", "sing_exact_multi", "gsva_kcdf_table",
    "plaid_test_multi", "shard_bounds", "multi_finalize", "replaid_ucell_exact", "replaid_aucell_exact", "ucell_exact_multi",
    "aucell_exact_multi", "plaid_test_contrasts", "plaid_test_contrasts_multi", "plaid_gsea", "gsea_multi", "gsea_multilevel_multi",
    "plaid_fisher", "plaid_sig", "fisher_multi", "plaid_limma", "plaid_limma_contrasts", "limma_multi", "plaid_voom", "voom_multi",
    "plaid_rankcor", "rankcor_multi", "replaid_plage", "replaid_zscore", "plage_multi", "zscore_multi",
    "plaid_camera", "plaid_camera_contrasts", "plaid_intergenecor", "camera_multi",
    "plaid_fry", "plaid_fry_contrasts", "fry_multi",
    "plaid_roast", "plaid_roast_contrasts", "roast_multi",
    "plaid_romer", "plaid_romer_contrasts", "romer_multi",
]
__version__ = "0.2.0"
