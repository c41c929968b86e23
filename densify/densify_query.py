from dhr_amd.densify_sparse import densify, whole_word_matching  # noqa: F401
from dhr_amd.densify_sparse import query_main as main

if __name__ == "__main__":
    main()
