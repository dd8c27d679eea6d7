"""The host files a stand-alone program over the tree-likelihood statements links (host/treelik*.cpp and what they call)."""
TREELIK_HOST_SOURCES = ("treelik.cpp", "treelik_rates.cpp", "treelik_anc.cpp", "treelik_nni.cpp", "treelik_support.cpp", "model_factory.cpp", "phytree.cpp", "alphabet.cpp",
                        "host_threads.cpp")
