"""Drop-in module path of the reference (`python -m densify.densify_corpus`, `python -m densify.densify_query`):
thin aliases of dhr_amd.densify_sparse."""
