"""python -m experiments.training.front_L41V2 -- see experiments/training/_recipes.py."""
from experiments.training._recipes import main

if __name__ == '__main__':
    main('front_L41V2')
