from dhr_amd.densify_sparse import densify, get_files, omission_num, vectorize_and_densify, whole_word_matching  # noqa: F401
from dhr_amd.densify_sparse import corpus_main as main

if __name__ == "__main__":
    main()
